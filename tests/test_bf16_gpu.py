"""precision = 1 (bf16 storage, fp32 accumulate; BASELINE.json configs[2..3]) parity tests.

Operator level: inputs and weights are rounded to bf16 on the host first, so the comparison with the
fp64 oracle isolates the kernel (fp32 accumulation + one bf16 rounding of the output):
    |gpu - ref| <= 2^-8 * max(1, |ref|_inf)          (bf16 outputs; 2^-9 is half an ulp at the top binade)
    |gpu - ref| <= 2e-4 * max(1, |ref|_inf)          (fp32 outputs of the bf16 kernels: eps / RGB heads)
Model level (full-width UNet / decoder at an 8x8 latent): relative RMS error against the fp64 oracle on
the un-rounded weights; bars set from the first measurements ("expect ~1e-2 bf16").
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def bf16_round(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def _t(a):
    return torch.from_numpy(np.asarray(a)).double()


def _check(got, ref, what, rel):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = np.abs(got - ref).max()
    bound = rel * max(1.0, np.abs(ref).max())
    assert err <= bound, f"{what}: max|d|={err:.3e} > {bound:.3e} (rms {np.sqrt(np.mean((got - ref) ** 2)):.3e})"


@pytest.fixture(scope="module")
def ops16():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=1))
    yield sd
    sd.close()


CONV16 = [
    (2, 320, 16, 16, 320, 3, 1, 0), (1, 640, 8, 8, 640, 3, 1, 1), (2, 320, 16, 16, 320, 3, 2, 0),
    (2, 640, 16, 16, 320, 1, 1, 0), (1, 2560, 8, 8, 1280, 3, 1, 0), (1, 256, 24, 40, 128, 3, 1, 0),
    (1, 320, 16, 16, 4, 3, 1, 0),     # eps head: bf16 kernel, fp32 output
    (1, 128, 16, 16, 3, 3, 1, 0),     # RGB head: N = 3, fp32 output
    (1, 4, 16, 16, 320, 3, 1, 0),     # conv_in: fp32 kernel (Cin = 4) emitting bf16
    (3, 64, 5, 7, 96, 3, 1, 0),
]


@pytest.mark.parametrize("case", CONV16)
def test_conv2d_bf16(ops16, case):
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(hash(case) % (2 ** 31))
    x = g.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k)).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    if cin % 64 == 0:   # the kernel sees bf16 operands
        x, wt = bf16_round(x), bf16_round(wt)
    got = ops16.op_conv2d(x, wt, b, stride=stride, upsample2x=bool(ups))
    xin = O.upsample2x(_t(x)) if ups else _t(x)
    ref = O.conv2d(xin, (_t(wt), _t(b)), stride=stride, padding=1 if k == 3 else 0).numpy()
    _check(got, ref, f"conv2d bf16 {case}", 2e-4 if cout <= 4 else 2 ** -8)


@pytest.mark.parametrize("tile", range(10))
@pytest.mark.parametrize("splitk", [1, 3])
def test_conv2d_bf16_all_tiles(ops16, tile, splitk):
    n, cin, h, w, cout = 2, 128, 13, 11, 208
    g = np.random.default_rng(2000 + tile)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", splitk)
        got = ops16.op_conv2d(x, wt, b)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    ref = O.conv2d(_t(x), (_t(wt), _t(b)), padding=1).numpy()
    _check(got, ref, f"conv bf16 tile={tile} splitk={splitk}", 2 ** -8)


XCASES = [
    # (n, cin, h, w, cout, k, stride, ups): several M tiles with a ragged last one, N tails, every conv flavour
    (2, 128, 23, 19, 320, 3, 1, 0), (1, 64, 40, 36, 200, 3, 1, 0), (2, 192, 16, 16, 640, 1, 1, 0), (1, 128, 33, 31, 128, 3, 2, 0),
    (1, 64, 12, 20, 384, 3, 1, 1),
]


@pytest.mark.parametrize("tile", [100, 101, 102, 103])
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("case", XCASES)
def test_conv2d_bf16_large_tiles(ops16, tile, splitk, case):
    """k_gemm_bf16x.hip: 256-row, 8-wave tiles staged by LDS-DMA (tile 100 + x), incl. residual + time-embedding epilogue."""
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(3000 + tile + 7 * splitk + cin + cout)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", splitk)
        got = ops16.op_conv2d(x, wt, b, stride=stride, upsample2x=bool(ups))
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    xin = O.upsample2x(_t(x)) if ups else _t(x)
    ref = O.conv2d(xin, (_t(wt), _t(b)), stride=stride, padding=1 if k == 3 else 0).numpy()
    _check(got, ref, f"conv bf16 large tile={tile} splitk={splitk} {case}", 2 ** -8)


XCASES_SHORT_K = [
    # (n, cin, h, w, cout, k, splitk): one to three 64-channel k tiles per slice
    (1, 64, 16, 16, 320, 1, 1), (1, 128, 16, 16, 320, 1, 1), (1, 128, 16, 16, 320, 1, 2), (2, 64, 9, 9, 128, 3, 9), (2, 64, 9, 9, 128, 3, 3), (1, 192, 20, 20, 200, 1, 1),
]


@pytest.mark.parametrize("tile", [100, 101])
@pytest.mark.parametrize("case", XCASES_SHORT_K)
def test_conv2d_bf16_large_tiles_short_k(ops16, tile, case):
    """one to three k tiles per k slice"""
    n, cin, h, w, cout, k, splitk = case
    g = np.random.default_rng(3100 + tile + cin + cout + splitk)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", splitk)
        got = ops16.op_conv2d(x, wt, b)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    ref = O.conv2d(_t(x), (_t(wt), _t(b)), padding=1 if k == 3 else 0).numpy()
    _check(got, ref, f"conv bf16 large tile={tile} short K {case}", 2 ** -8)


TCASES = [
    # (n, cin, h, w, cout, splitk): 3x3 / stride 1 / pad 1, widths 16 ... 128, pixel counts that are multiples of the 256-row tile, k slices of whole kernel rows
    (2, 128, 16, 16, 320, 1), (1, 64, 32, 32, 256, 1), (1, 64, 64, 64, 96, 1), (1, 64, 16, 128, 64, 1), (3, 192, 16, 16, 328, 3), (2, 128, 32, 32, 640, 2),
    (1, 64, 32, 16, 48, 3), (1, 320, 64, 64, 320, 1),
]


@pytest.mark.parametrize("tile", [104, 105])
@pytest.mark.parametrize("case", TCASES)
def test_conv2d_bf16_kernel_row_tiles(ops16, tile, case):
    """k_gemm_bf16t.hip: the three taps of a kernel row read from one staged activation tile (image rows padded in LDS, border columns from the zero page);
    the reference launch is the forced plain tile 100 / 101 -- a forced tile is not upgraded to the kernel-row form"""
    n, cin, h, w, cout, splitk = case
    g = np.random.default_rng(3300 + tile + cin + cout + splitk + w)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, 3, 3)) / math.sqrt(cin * 9))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", splitk)
        got = ops16.op_conv2d(x, wt, b)
        ops16.set_option("gemm_tile", tile - 4)
        same = ops16.op_conv2d(x, wt, b)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
    ref = O.conv2d(_t(x), (_t(wt), _t(b)), padding=1).numpy()
    _check(got, ref, f"conv bf16 kernel-row tile={tile} {case}", 2 ** -8)
    # the same products in the same order as the tile it replaces: bit-identical
    np.testing.assert_array_equal(got, same)


def test_conv2d_bf16_kernel_row_tiles_refuse_other_layers(ops16):
    g = np.random.default_rng(5)
    x = bf16_round(g.standard_normal((1, 64, 8, 8)))
    wt = bf16_round(g.standard_normal((64, 64, 3, 3)) / 24.0)
    try:
        ops16.set_option("gemm_tile", 104)
        with pytest.raises(Exception):
            ops16.op_conv2d(x, wt, None)
    finally:
        ops16.set_option("gemm_tile", "auto")


@pytest.mark.parametrize("tile", [100, 103])
def test_linear_bf16_large_tiles(ops16, tile):
    g = np.random.default_rng(tile)
    rows, cin, cout = 700, 320, 960
    x = bf16_round(g.standard_normal((rows, cin)))
    wt = bf16_round(g.standard_normal((cin, cout)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        got = ops16.op_linear(x, wt, b)
    finally:
        ops16.set_option("gemm_tile", "auto")
    _check(got, O.linear(_t(x), _t(wt), _t(b)).numpy(), f"linear bf16 large tile={tile}", 2 ** -8)


@pytest.mark.parametrize("rows,cin,cout", [(154, 768, 320), (512, 320, 2560), (77, 64, 192), (1, 1280, 1280)])
def test_linear_bf16(ops16, rows, cin, cout):
    g = np.random.default_rng(rows + cout)
    x = bf16_round(g.standard_normal((rows, cin)))
    wt = bf16_round(g.standard_normal((cin, cout)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    got = ops16.op_linear(x, wt, b)
    _check(got, O.linear(_t(x), _t(wt), _t(b)).numpy(), f"linear bf16 ({rows},{cin},{cout})", 2 ** -8)


@pytest.mark.parametrize("n,c,h,w", [(2, 320, 16, 16), (1, 1920, 8, 8), (1, 128, 32, 32), (2, 2560, 8, 8), (2, 640, 1, 1)])
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm_bf16(ops16, n, c, h, w, silu):
    g = np.random.default_rng(c + h)
    x = bf16_round(g.standard_normal((n, c, h, w)) * 1.7 + 0.9)
    gamma = (1 + 0.1 * g.standard_normal(c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c)).astype(np.float32)
    got = ops16.op_group_norm(x, gamma, beta, 32, 1e-5, silu)
    ref = O.group_norm(_t(x), _t(gamma), _t(beta), 32, 1e-5)
    if silu:
        ref = O.silu(ref)
    _check(got, ref.numpy(), f"group_norm bf16 {(n, c, h, w)} silu={silu}", 2 ** -8)


@pytest.mark.parametrize("rows,c", [(64, 320), (257, 640), (33, 1280)])
def test_layer_norm_bf16(ops16, rows, c):
    g = np.random.default_rng(rows)
    x = bf16_round(g.standard_normal((rows, c)) * 2 - 0.5)
    gamma = (1 + 0.1 * g.standard_normal(c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c)).astype(np.float32)
    got = ops16.op_layer_norm(x, gamma, beta, 1e-5)
    _check(got, O.layer_norm(_t(x), _t(gamma), _t(beta), 1e-5).numpy(), f"layer_norm bf16 ({rows},{c})", 2 ** -8)


def test_geglu_bf16(ops16):
    g = np.random.default_rng(3)
    proj = bf16_round(g.standard_normal((37, 2 * 640)) * 2)
    got = ops16.op_geglu(proj)
    p = _t(proj)
    _check(got, (p[:, :640] * O.gelu_erf(p[:, 640:])).numpy(), "geglu bf16", 2 ** -8)


@pytest.mark.parametrize("case", [(2, 256, 256, 320, 8), (2, 64, 64, 640, 8), (1, 256, 256, 1280, 8), (2, 256, 77, 320, 8),
                                  (2, 64, 2, 1280, 8), (3, 2048, 512, 320, 8), (1, 64, 64, 256, 1),
                                  (4, 2048, 192, 320, 8), (2, 50, 100, 640, 8), (1, 300, 333, 1280, 8), (2, 1024, 1024, 640, 8)])
@pytest.mark.parametrize("mfma16", [1, 0])
def test_qkv_attention_bf16(ops16, case, mfma16):
    """mfma16 = 1: bf16 matrix-core kernel (k_attn_bf16.hip; probabilities rounded to bf16 for P V);
    0: bf16 storage widened onto the fp32 kernel."""
    n, nq, nk, c, heads = case
    ops16.set_option("attn_bf16", mfma16)
    g = np.random.default_rng(hash(case) % (2 ** 31))
    q, k, v = (bf16_round(g.standard_normal((n, s, c))) for s in (nq, nk, nk))
    got = ops16.qkv_attention(q, k, v, None, heads)
    ref = O.qkv_attention(_t(q), _t(k), _t(v), None, heads).numpy()
    # fused path: fp32 math on bf16 inputs, bf16 output; unfused (1 head): probabilities are rounded to bf16 too.  At this fp32 boundary q is
    # multiplied by d^-0.5 log2(e) and rounded to bf16 ONCE MORE (the kernels take q in log2 units; inside the model that factor sits in the
    # query weights and costs no rounding): 2^-7 instead of 2^-8 for the fused kernels
    _check(got, ref, f"qkv_attention bf16 {case}", 2 ** -7 if heads > 1 else 2 ** -6)


@pytest.mark.parametrize("case", [(2, 256, 256, 320, 8), (2, 256, 77, 320, 8), (3, 2048, 512, 320, 8), (4, 2048, 192, 320, 8), (2, 50, 100, 320, 8), (1, 300, 333, 320, 8),
                                  (2, 64, 2, 320, 8), (1, 700, 130, 320, 8), (2, 1024, 1024, 640, 8), (2, 50, 100, 640, 8)])
@pytest.mark.parametrize("variant", [1, 2, 4])
def test_qkv_attention_bf16_variants(ops16, case, variant):
    """Round 6, option attn_bf16_variant (k_attn_bf16.hip): bit 0 = two 4-wave workgroups per CU, bit 1 = 64 query rows per wave (two score blocks sharing every K / V^T fragment)
    on 8-wave workgroups, bit 2 = the same on 4-wave workgroups; 0x100 forces the form whatever the grid.  Same products and the same per-row softmax as the default form
    (the two-block forms walk 64-key tiles instead of 128-key ones, so a row's reference maximum may move at other keys): the operator's 2^-7 bar against the oracle, and
    agreement with the default form to the same bar.  Ragged query and key counts, one-tile and two-key contexts included; head dims without the form fall back to the default."""
    n, nq, nk, c, heads = case
    ops16.set_option("attn_bf16", 1)
    g = np.random.default_rng(hash(case) % (2 ** 31))
    q, k, v = (bf16_round(g.standard_normal((n, s, c))) for s in (nq, nk, nk))
    ref = O.qkv_attention(_t(q), _t(k), _t(v), None, heads).numpy()
    try:
        ops16.set_option("attn_bf16_variant", 0)
        base = ops16.qkv_attention(q, k, v, None, heads)
        ops16.set_option("attn_bf16_variant", 0x100 | variant)
        got = ops16.qkv_attention(q, k, v, None, heads)
    finally:
        ops16.set_option("attn_bf16_variant", "default")
    _check(got, ref, f"qkv_attention bf16 variant {variant} {case}", 2 ** -7)
    assert np.abs(got.astype(np.float64) - base.astype(np.float64)).max() <= 2 ** -7 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("variant", [0, 0x102, 0x104])
@pytest.mark.parametrize("case", [(2, 512, 1024, 320, 8), (1, 256, 700, 640, 8), (1, 128, 512, 1280, 8)])
@pytest.mark.parametrize("gain", [4.0, 12.0])
def test_qkv_attention_bf16_moving_maximum(ops16, case, gain, variant):
    """k_attn_bf16.hip raises its reference maximum only when a tile's maximum exceeds it by 2^8: keys ordered so that the row maxima keep
    growing tile after tile (every tile takes the rescale path at gain 12, some at gain 4), scores spread over tens of log2 units.  Rows are
    nearly one-hot here, so the oracle is given exactly the q the kernel multiplies -- bf16(q d^-0.5 log2 e), what the boundary's conversion
    produces (the rounding of that conversion is test_qkv_attention_bf16's subject) -- and the bar is the fused kernels' 2^-8."""
    n, nq, nk, c, heads = case
    if variant and c // heads != 40:
        pytest.skip("the two-block forms are d = 40 instantiations")
    ops16.set_option("attn_bf16", 1)
    ops16.set_option("attn_bf16_variant", variant)
    g = np.random.default_rng(int(gain) + nk)
    q = bf16_round(g.standard_normal((n, nq, c)))
    k = bf16_round(g.standard_normal((n, nk, c)) * np.linspace(0.2, gain, nk)[None, :, None])      # later keys score higher in magnitude
    v = bf16_round(g.standard_normal((n, nk, c)))
    got = ops16.qkv_attention(q, k, v, None, heads)
    f = np.float32(1.4426950408889634 / math.sqrt(c // heads))       # kernels.hpp attn_bf16_q_scale
    q_seen = bf16_round(q * f).astype(np.float64) / np.float64(f)
    ref = O.qkv_attention(_t(q_seen), _t(k), _t(v), None, heads).numpy()
    ops16.set_option("attn_bf16_variant", "default")
    assert np.isfinite(got).all()
    _check(got, ref, f"qkv_attention bf16 moving maximum {case} gain={gain}", 2 ** -8)


@pytest.mark.parametrize("rows,cin,hidden", [(700, 320, 1280), (2048, 320, 1280), (513, 128, 384)])
@pytest.mark.parametrize("fuse", [2, 3, 0])   # 2 / 3: fused, 256x128 / 256x256 tiles; 0: GEMM + gate kernel
def test_geglu_forward_bf16(ops16, rows, cin, hidden, fuse):
    g = np.random.default_rng(rows + hidden + fuse)
    x = bf16_round(g.standard_normal((rows, cin)))
    w = bf16_round(g.standard_normal((cin, 2 * hidden)) / math.sqrt(cin))
    b = g.standard_normal(2 * hidden).astype(np.float32)
    try:
        ops16.set_option("geglu_fuse", fuse)
        got = ops16.op_geglu_forward(x, w, b, hidden)
    finally:
        ops16.set_option("geglu_fuse", 1)
    proj = _t(x) @ _t(w) + _t(b)
    ref = (proj[:, :hidden] * O.gelu_erf(proj[:, hidden:])).numpy()
    # unfused: the projection is rounded to bf16 before the gate (one more rounding than the fused form)
    _check(got, ref, f"geglu_forward bf16 ({rows},{cin},{hidden}) fuse={fuse}", 2 ** -8 if fuse else 2 ** -7)


# ---- round 5: the persistent tile loop (gemm_bf16x_variant bit 0, the default) ------------------------------------------------------------------------------------
# It keeps every product, its order and the single rounding: results must be BIT-IDENTICAL to variant 0 (one tile per workgroup), which the tests above hold against
# the oracle.  The shapes have more tiles than the chip has CUs (the persistent form's condition), ragged M, N tails, one to twenty k tiles, padding taps in a tile's
# FIRST k tile (issue_first); a residual launch takes the loop too when its residual is in the accumulators (resid_acc bit 0, the default; round 6), else the one-tile form.  (Round 5 also measured an epilogue without the LDS
# transpose -- v_permlane16_swap pairs, 64-byte row pieces -- bit-identical and 4 ... 7 % slower per launch: removed, profiles/r05a_*.)
def _variants(ops16, fn, what, variants=(1, 4, 5, 8, 13)):     # bit 0: persistent tile loop (round 5); bit 2: staggered DMA issue of the two wave groups (round 6); 5 = the default; bit 3: the GENERAL epilogue on interior tiles too (round 6: variant 0 and the default take the lean one)
    try:
        ops16.set_option("gemm_bf16x_variant", 0)
        base = fn()
        for v in variants:
            ops16.set_option("gemm_bf16x_variant", v)
            got = fn()
            assert np.isfinite(got).all(), f"{what} variant {v}"
            np.testing.assert_array_equal(got, base, err_msg=f"{what}: gemm_bf16x_variant={v} differs from 0")
    finally:
        ops16.set_option("gemm_bf16x_variant", "default")
    return base


PERSIST_LINEAR = [(70001, 64, 1000), (70001, 320, 960), (33000, 128, 2560), (66000, 1280, 320), (140000, 320, 320)]


@pytest.mark.parametrize("tile", [100, 101, 102, 103])
@pytest.mark.parametrize("rows,cin,cout", PERSIST_LINEAR)
@pytest.mark.parametrize("resid", [0, 1])
def test_linear_bf16_persistent_and_direct_epilogue(ops16, tile, rows, cin, cout, resid):
    if resid and cin != cout:
        pytest.skip("the residual test form needs cin == cout")
    g = np.random.default_rng(5000 + tile + rows + cin + cout)
    x = bf16_round(g.standard_normal((rows, cin)))
    wt = bf16_round(g.standard_normal((cin, cout)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("op_resid", resid)
        base = _variants(ops16, lambda: ops16.op_linear(x, wt, b), f"linear ({rows},{cin},{cout}) tile={tile} resid={resid}")
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("op_resid", 0)
    rs = np.r_[0:300, rows // 2:rows // 2 + 300, rows - 300:rows]     # oracle on the first / middle / last rows (a full fp64 product would take longer than the rest of the file)
    ref = O.linear(_t(x[rs]), _t(wt), _t(b)).numpy() + (x[rs] if resid else 0.0)
    _check(base[rs], ref, f"linear bf16 persistent shapes ({rows},{cin},{cout}) tile={tile} resid={resid}", 2 ** -8)


@pytest.mark.parametrize("case", [(8, 64, 97, 97, 320, 3, 1, 0), (8, 64, 49, 48, 200, 3, 1, 1), (8, 128, 96, 96, 64, 1, 1, 0), (8, 64, 96, 96, 64, 3, 1, 0)])
@pytest.mark.parametrize("tile", [100, 101, 102])
def test_conv2d_bf16_persistent_and_direct_epilogue(ops16, tile, case):
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(5100 + tile + cin + cout + h)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k))
    b = g.standard_normal(cout).astype(np.float32)
    resid = int(cin == cout)
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("op_resid", resid)
        base = _variants(ops16, lambda: ops16.op_conv2d(x, wt, b, stride=stride, upsample2x=bool(ups)), f"conv {case} tile={tile}")
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("op_resid", 0)
    xin = O.upsample2x(_t(x[:1])) if ups else _t(x[:1])               # oracle on the first sample
    ref = O.conv2d(xin, (_t(wt), _t(b)), stride=stride, padding=1 if k == 3 else 0).numpy() + (x[:1] if resid else 0.0)
    _check(base[:1], ref, f"conv bf16 persistent shapes {case} tile={tile}", 2 ** -8)


@pytest.mark.parametrize("rows,cin,hidden", [(40000, 320, 1280), (70001, 64, 328)])
@pytest.mark.parametrize("fuse", [2, 3])
def test_geglu_forward_bf16_persistent_and_direct_epilogue(ops16, rows, cin, hidden, fuse):
    g = np.random.default_rng(5200 + rows + hidden + fuse)
    x = bf16_round(g.standard_normal((rows, cin)))
    w = bf16_round(g.standard_normal((cin, 2 * hidden)) / math.sqrt(cin))
    b = g.standard_normal(2 * hidden).astype(np.float32)
    try:
        ops16.set_option("geglu_fuse", fuse)
        base = _variants(ops16, lambda: ops16.op_geglu_forward(x, w, b, hidden), f"geglu_forward ({rows},{cin},{hidden}) fuse={fuse}")
    finally:
        ops16.set_option("geglu_fuse", 1)
    rs = np.r_[0:300, rows - 300:rows]
    proj = _t(x[rs]) @ _t(w) + _t(b)
    _check(base[rs], (proj[:, :hidden] * O.gelu_erf(proj[:, hidden:])).numpy(), f"geglu_forward bf16 persistent shapes ({rows},{cin},{hidden}) fuse={fuse}", 2 ** -8)


# ---- model level: full-width UNet / decoder at an 8x8 latent -----------------------------------------------------
@pytest.fixture(scope="module")
def sd16():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(320, 8, 768, 8, 8, 64, precision=1))
    sd.load_weights(syn.SyntheticWeights())
    yield sd
    sd.close()


DIMS16 = O.Dims(320, 8, 768, 8, 8, 64)


# model-level bars = 1.5 x the relative RMS measured on MI355X (UNet forward 1.1e-2, 5-step CFG latent 1.7e-2, decoded RGB 0.9e-2)
BAR_UNET, BAR_LATENT, BAR_RGB = 1.7e-2, 2.6e-2, 1.4e-2


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


@functools.lru_cache(maxsize=None)
def _unet_oracle64(t):
    """the fp64 oracle's UNet forward on the two test latents at timestep t (seconds of host time: shared by the tests that need it)"""
    lat = np.stack([syn.initial_latent(i, 8, 8) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 77, 768) for i in range(2)])
    return O.UNetOracle(syn.SyntheticWeights(), DIMS16, torch.float64).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx)).numpy()


def test_unet_forward_bf16(sd16):
    lat = np.stack([syn.initial_latent(i, 8, 8) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 77, 768) for i in range(2)])
    got = sd16.unet.forward(lat, [999], ctx)
    ref = _unet_oracle64(999)
    r = _rel_rms(got, ref)
    print(f"bf16 UNet forward: rel-RMS vs fp64 oracle = {r:.3e}, max|d| = {np.abs(got - ref).max():.3e} (|ref|max {np.abs(ref).max():.2f})")
    assert np.isfinite(got).all() and r < BAR_UNET


@pytest.mark.parametrize("tile", [100, 103])
def test_unet_forward_bf16_large_tiles_forced(sd16, tile):
    """every bf16 GEMM of the UNet on a k_gemm_bf16x.hip tile: covers its residual / time-embedding / split-K epilogues."""
    lat = np.stack([syn.initial_latent(i, 8, 8) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 77, 768) for i in range(2)])
    base = sd16.unet.forward(lat, [500], ctx)
    try:
        sd16.set_option("gemm_tile", tile)
        got = sd16.unet.forward(lat, [500], ctx)
    finally:
        sd16.set_option("gemm_tile", "auto")
    ref = _unet_oracle64(500)
    r, r0 = _rel_rms(got, ref), _rel_rms(base, ref)
    print(f"bf16 UNet forward, tile {tile} forced: rel-RMS {r:.3e} (auto tiles {r0:.3e})")
    assert np.isfinite(got).all() and r < BAR_UNET


def test_sample_image_bf16(sd16):
    lat = syn.initial_latent(0, 8, 8)[None]
    ctx = syn.cond_context(0, 77, 768)[None]
    unc = syn.uncond_context(77, 768)
    a = syn.alphas_cumprod()
    o64 = O.StableDiffusionOracle(syn.SyntheticWeights(), a, DIMS16, torch.float64)
    got = sd16.sample_latent(ctx, unc, 7.5, 5, init_latent=lat)
    ref = o64.sample_latent(torch.from_numpy(ctx), torch.from_numpy(unc), 7.5, 5, torch.from_numpy(lat)).numpy()
    r = _rel_rms(got, ref)
    print(f"bf16 sample_latent (5 steps, CFG 7.5): rel-RMS = {r:.3e}")
    assert np.isfinite(got).all() and r < BAR_LATENT
    img = sd16.autoencoder.decode_latent((ref * (1.0 / 0.18215)).astype(np.float32))
    ref_img = o64.decoder.decode_latent(torch.from_numpy(ref) * (1.0 / 0.18215)).numpy()
    r2 = _rel_rms(img, ref_img)
    print(f"bf16 decode_latent: rel-RMS = {r2:.3e}")
    assert np.isfinite(img).all() and r2 < BAR_RGB
    u8 = sd16.sample_image(ctx, unc, 7.5, 5, init_latent=lat)
    assert u8.shape == (1, 64, 64, 3) and u8.dtype == np.uint8
    # the u8 image against the fp64 oracle's own image (truncating cast, stablediffusion/mod.rs:96): bf16 moves a pixel by a
    # few LSB, never by a visible amount
    ref_u8 = np.clip((np.transpose(ref_img, (0, 2, 3, 1)) + 1.0) / 2.0 * 255.0, 0.0, 255.0).astype(np.uint8)   # stablediffusion/mod.rs:79-99, truncating
    du8 = np.abs(u8.astype(np.int16) - ref_u8.astype(np.int16))
    print(f"bf16 u8 image vs fp64 oracle: mean |d| = {du8.mean():.2f} LSB, max = {du8.max()} LSB")
    assert du8.mean() < 4.0 and du8.max() <= 40


def test_bf16_batch_and_repeatability(sd16):
    lat = np.stack([syn.initial_latent(i, 8, 8) for i in range(2)])
    ctx = np.stack([syn.cond_context(i, 77, 768) for i in range(2)])
    unc = syn.uncond_context(77, 768)
    a = sd16.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    b = sd16.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    assert np.array_equal(a, b)
