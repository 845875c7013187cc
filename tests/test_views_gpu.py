"""Channel-slice views: the UNet realises Tensor::cat (unet/mod.rs:134) without a copy -- the input of output block i is one buffer [x channels | skip
channels], every block's last kernel writes a slice of it (ldc > N, base at a channel offset, live data in the neighbouring columns) and every input
block after the first reads one (ldx / a_ld > C).  The sdmi_op_*_view entries run convolution, Linear and GroupNorm that way, through Engine::slice and
the engine's own conv / conv_fp8 / gemm / gemm_fp8 / group_norm / group_norm_fp8 / quantize.

Every case here holds
  * the slice to the fp64 oracle of the dense operation at the operator bars of its precision (2e-5 max(1, |ref|) at precision 0, 2^-8 max(1, |ref|)
    for bf16 outputs, the MXFP8 GroupNorm bars of test_fp8_gpu.py) -- the input parent's other columns are NaN, so a read over the edge is a NaN;
  * every element of the output parent outside the slice to its prefill, BIT FOR BIT -- the prefill is a position-dependent pattern of values exact in
    bf16, so a store that is shifted, duplicated or one vector too long shows;
  * the slice to the dense entry's result bit for bit wherever dump_choices records the same launch (kernel, tile, split count, resid_acc bits) for the
    two; where the record differs the test names the gate that made it differ (set_resid_acc's ldc % 8).
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
NAN = float("nan")

# the model's own cuts (cx, cskip): full width, then the half-width model's
MODEL_CUTS = [(320, 320), (640, 320), (640, 640), (1280, 640), (1280, 1280), (160, 160), (320, 160)]


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
    assert np.isfinite(got).all(), f"{what}: non-finite output (a neighbour column of the input read?)"
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


_DEFAULTS = {"gemm_tile": "auto", "splitk": 0, "resid_acc": 3, "fp8_tile": "auto", "fp8_ops": 0, "gemm_bf16x_variant": "default", "gemm3x_variant": "default",
             "gemm_planes": "default", "gn32_min_wgs": 256, "gn32_stats_min_wgs": 64, "gn_target_wgs": 512, "gn_unroll": 2}


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


def _splits(case, splitk, kt_elems):
    """the split count launch_gemm makes of a forced `splitk`: at most one per k tile (128 bytes of K per row), slices of equal length"""
    kt = -(-(case[1] * case[5] * case[5]) // kt_elems)
    s = max(1, min(splitk, kt))
    per = -(-kt // s)
    return -(-kt // per)


def _took(lines, what, cfg=None, splits=None):
    assert len(lines) == 1, f"{what}: expected one GEMM launch, got {lines}"
    if cfg is not None:
        assert f" cfg={cfg} " in lines[0], f"{what}: tile not taken: {lines[0]}"
    if splits is not None:
        assert f" splits={splits} " in lines[0], f"{what}: split count not taken: {lines[0]}"


# ---- parents: prefill, slicing, the neighbour check ----------------------------------------------------------------------------------------------------------
def _prefill(rows, ld):
    """position-dependent, every value a multiple of 1/4 below 32 in magnitude: exact in bf16 (and in the three-plane split), no two neighbours equal"""
    r = np.arange(rows, dtype=np.int64)[:, None]
    j = np.arange(ld, dtype=np.int64)[None, :]
    return (((r * 131 + j * 7) % 251 - 125) / 4.0).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _neighbours_intact(parent, pre, off, c, what):
    """every element outside columns [off, off + c) equals its prefill bit for bit"""
    assert parent.shape == pre.shape, what
    keep = np.ones(pre.shape[1], bool)
    keep[off:off + c] = False
    bad = _bits(parent)[:, keep] != _bits(pre)[:, keep]
    if bad.any():
        r, j = np.argwhere(bad)[0]
        col = np.flatnonzero(keep)[j]
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the slice [{off}, {off + c}) of {pre.shape[1]} changed; first at row {r} column {col}: "
                             f"{parent[r, col]!r} (prefill {pre[r, col]!r})")


def _nchw(parent, off, c, n, ho, wo):
    return np.ascontiguousarray(parent[:, off:off + c].reshape(n, ho, wo, c).transpose(0, 3, 1, 2))


def _out_hw(h, w, k, stride, ups):
    pad = 1 if k == 3 else 0
    return ((h << ups) + 2 * pad - k) // stride + 1, ((w << ups) + 2 * pad - k) // stride + 1


# ---- operands and fp64 references, cached per shape -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_case(case, fmt):
    """x, weight, bias, per-sample temb, residual and the fp64 conv(x) (no bias) of one shape; fmt 'f32', 'bf16' (operands rounded to bf16) or 'mx' (operands
    on the MX grid); the residual is bf16-rounded at bf16 / MX"""
    n, cin, h, w, cout, k, stride, ups = case
    g = np.random.default_rng(zlib.crc32(repr((case, fmt, "views")).encode()))
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
    resid = g.standard_normal((n, cout, ho, wo)).astype(np.float32)
    if fmt != "f32":
        resid = bf16_round(resid)
    xin = O.upsample2x(_t(x)) if ups else _t(x)
    conv = O.conv2d(xin, (_t(wt), None), stride=stride, padding=1 if k == 3 else 0).numpy()
    return x, wt, b, temb, resid, conv


def _ref(conv, bias=None, temb=None, resid=None):
    r = conv.copy()
    if bias is not None:
        r += np.asarray(bias, np.float64)[None, :, None, None]
    if temb is not None:
        r += np.asarray(temb, np.float64)[:, :, None, None]
    if resid is not None:
        r += resid
    return r


def _conv_view(sd, tmp_path, case, c, epi, view, opts, what, bar, dense=None, gate=None):
    """one convolution into the slice `view` = (out_off, out_ld, in_off, in_ld, in_planes, out_planes): oracle, neighbours, and bit identity with the dense
    result `dense` = (array, dump_choices lines) where the records agree.  Returns (slice as NCHW, lines)."""
    n, cin, h, w, cout, k, stride, ups = case
    x, wt, b, temb, resid, conv = c
    out_off, out_ld, in_off, in_ld, in_planes, out_planes = view
    ho, wo = _out_hw(h, w, k, stride, ups)
    pre = _prefill(n * ho * wo, out_ld)
    bias, tm, rs = (b, temb, resid) if epi else (None, None, None)
    rld = (cout + 24) if epi else 0      # the residual keeps a stride of its own, NaN padded (test_epilogue_gpu.py)
    got, lines = _run(sd, tmp_path, lambda: sd.op_conv2d_view(x, wt, bias, tm, rs, stride=stride, upsample2x=bool(ups), resid_ld=rld, parent=pre, out_off=out_off,
                                                              in_ld=in_ld, in_off=in_off, in_planes=in_planes, out_planes=out_planes), **opts)
    parents = got if isinstance(got, tuple) else (got,)
    for i, p in enumerate(parents):
        _neighbours_intact(p, pre, out_off, cout, f"{what} (copy {i})")
    if len(parents) == 2:
        assert np.array_equal(_bits(parents[0]), _bits(parents[1])), f"{what}: the fp32 and the plane copy of the output differ"
    y = _nchw(parents[0], out_off, cout, n, ho, wo)
    _check(y, _ref(conv, bias, tm, rs), what, bar)
    if dense is not None:
        dy, dlines = dense
        if lines == dlines:
            assert np.array_equal(_bits(y), _bits(dy)), f"{what}: same launch record as the dense call ({lines}) but different bits"
        else:
            assert gate is not None and gate(lines, dlines), f"{what}: launch record differs from the dense call's for no named reason: {lines} vs {dlines}"
    return y, lines


def _dense_conv(sd, tmp_path, case, c, epi, opts):
    n, cin, h, w, cout, k, stride, ups = case
    x, wt, b, temb, resid, conv = c
    bias, tm, rs = (b, temb, resid) if epi else (None, None, None)
    return _run(sd, tmp_path, lambda: sd.op_conv2d_epilogue(x, wt, bias, tm, rs, stride=stride, upsample2x=bool(ups), resid_ld=(cout + 24) if epi else 0), **opts)


def _acc_gate(ldc):
    """set_resid_acc (engine.cpp): resid_acc needs ldc % 8 == 0 -- a view whose parent is not a multiple of 8 wide adds bias / row / residual in the epilogue
    (acc=0) where the dense launch (ldc = N) starts the accumulators from them"""
    def gate(lines, dlines):
        strip = lambda ls: [ln.rsplit(" acc=", 1)[0] for ln in ls]
        return ldc % 8 != 0 and strip(lines) == strip(dlines) and all(" acc=0 " in ln + " " for ln in lines)
    return gate


def _planes_gate(lines, dlines):
    """launch_gemm (engine.cpp, from_planes): activations that ARRIVE as planes run on a plane tile (300 + x, from the plane table or its cost model), whatever
    tile the fp32 tables hold for the shape"""
    key = lambda ls: [ln.split(" cfg=")[0] for ln in ls]
    return key(lines) == key(dlines) and all(int(ln.split(" cfg=")[1].split()[0]) >= 300 for ln in lines)


# ---- 1. fp32: every tile of k_gemm.hip / k_gemm2.hip (0-9), k_gemm2x.hip (100-103), k_gemm3x.hip (200-205) writes and reads slices ---------------------------------
# (n, cin, h, w, cout, k, stride, ups): several M tiles with a ragged last one (XCASES of test_ops_gpu.py / test_planes_gpu.py), cout = 200 / 100: the last N tile of
# every tile shape (32 ... 320 columns) ends inside the parent
F32_CASES = [(2, 128, 23, 19, 200, 3, 1, 0), (1, 64, 40, 36, 200, 1, 1, 0), (1, 128, 33, 31, 100, 3, 2, 0), (1, 64, 12, 20, 200, 3, 1, 1)]
# (out_off, out_ld - cout - out_off, in_off, in_ld - cin - in_off): offsets / strides that are multiples of 32, of 8 but not 32, of 4 but not 8, and a stride off 4
# (ldc % 4 != 0: the scalar store forms; base still on 16 bytes)
F32_VIEWS = [(0, 320, 0, 320), (320, 0, 320, 0), (32, 32, 32, 64), (8, 16, 8, 8), (4, 8, 4, 4), (12, 8, 0, 0), (4, 6, 4, 8), (0, 2, 0, 4)]
F32_TILES = list(range(10)) + [100, 101, 102, 103] + [200, 201, 202, 203, 204, 205]


@pytest.mark.parametrize("case", F32_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", F32_TILES)
def test_conv_view_fp32_tiles(ops32, tmp_path, tile, splitk, case):
    n, cin, h, w, cout, k, stride, ups = case
    c = _conv_case(case, "f32")
    opts = dict(gemm_tile=tile, splitk=splitk)
    for epi in (False, True):
        dense = _dense_conv(ops32, tmp_path, case, c, epi, opts)
        _took(dense[1], f"dense {case} tile={tile}", tile, _splits(case, splitk, 32))
        for vi, (oo, opad, io, ipad) in enumerate(F32_VIEWS):
            if (vi + tile + splitk + int(epi)) % 2:      # half of the views per (tile, splitk, operands); every view meets every tile
                continue
            view = (oo, oo + cout + opad, io, io + cin + ipad, 0, 0)
            what = f"fp32 conv {case} tile={tile} splitk={splitk} epilogue={epi} view(out_off, out_ld, in_off, in_ld)={view[:4]}"
            _conv_view(ops32, tmp_path, case, c, epi, view, opts, what, FP32_BAR, dense)


# ---- 2. fp32 plane tiles (k_gemm3p.hip, 300-308): planes in, planes out, planes + fp32 out; the split-K reduce's plane-writing form ----------------------------------
P_CASES = [(2, 128, 23, 19, 160, 3, 1, 0), (1, 64, 40, 36, 320, 1, 1, 0), (1, 64, 33, 31, 160, 3, 2, 0), (1, 64, 12, 20, 160, 3, 1, 1)]
P_VIEWS = [(0, 160, 0, 64), (160, 0, 64, 0), (32, 64, 32, 32), (320, 0, 0, 0)]      # plane tensors are cut at multiples of 32 channels


@pytest.mark.parametrize("case", P_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", list(range(300, 309)))
def test_conv_view_fp32_plane_tiles(ops32, tmp_path, tile, splitk, case):
    n, cin, h, w, cout, k, stride, ups = case
    c = _conv_case(case, "f32")
    opts = dict(gemm_tile=tile, splitk=splitk)
    for epi in (False, True):
        dense = _dense_conv(ops32, tmp_path, case, c, epi, opts)
        _took(dense[1], f"dense {case} tile={tile}", tile, _splits(case, splitk, 32))
        for vi, (oo, opad, io, ipad) in enumerate(P_VIEWS):
            # input parent as fp32 (split in front of the launch), planes only, both; output parent as fp32, planes only (no residual: that needs fp32), both
            for fi, (inp, outp) in enumerate([(1, 1), (2, 3), (3, 2), (2, 1), (1, 3)]):
                if (vi + fi + tile + splitk) % 3 or (outp == 2 and epi):
                    continue
                view = (oo, oo + cout + opad, io, io + cin + ipad, inp, outp)
                what = f"fp32 conv {case} tile={tile} splitk={splitk} epilogue={epi} view={view[:4]} in_planes={inp} out_planes={outp}"
                _conv_view(ops32, tmp_path, case, c, epi, view, opts, what, FP32_BAR, dense)


# ---- 3. the model's own cuts at the tiles the tables / cost models choose, every precision ----------------------------------------------------------------------------
def _cut_case(cx, cskip, back, k):
    cout = cskip if back else cx
    return (2, 64, 13, 11, cout, k, 1, 0), ((cx if back else 0), cx + cskip)


@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("cut", MODEL_CUTS)
def test_conv_view_model_cuts_fp32(ops32, tmp_path, cut, back):
    """front slice (what output blocks and the middle block write) and back slice (what input blocks write); the parent exists as fp32 AND as planes, as unet_run
    allocates it (new_act3(..., 3)), read back from both"""
    for k in (3, 1):
        case, (off, ld) = _cut_case(*cut, back, k)
        c = _conv_case(case, "f32")
        for epi in (False, True):
            dense = _dense_conv(ops32, tmp_path, case, c, epi, {})
            for outp in (1, 3):
                what = f"fp32 conv {case} cut={cut} {'back' if back else 'front'} epilogue={epi} out_planes={outp}"
                _conv_view(ops32, tmp_path, case, c, epi, (off, ld, 0, 64, 0, outp), {}, what, FP32_BAR, dense)
    # and READ from the cut: the skip of the next input block (a_ld = ctot, base at cx / 0)
    cx, cskip = cut
    cin = cskip if back else cx
    case = (1, cin, 9, 7, 64, 1, 1, 0)
    c = _conv_case(case, "f32")
    dense = _dense_conv(ops32, tmp_path, case, c, False, {})
    for inp in (1, 3):
        _conv_view(ops32, tmp_path, case, c, False, (0, 64, cx if back else 0, cx + cskip, inp, 0), {}, f"fp32 conv {case} reading cut {cut} back={back} in_planes={inp}",
                   FP32_BAR, dense, _planes_gate if inp == 3 else None)


@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("cut", MODEL_CUTS)
def test_conv_view_model_cuts_bf16(ops16, tmp_path, cut, back):
    for k in (3, 1):
        case, (off, ld) = _cut_case(*cut, back, k)
        c = _conv_case(case, "bf16")
        for epi in (False, True):
            dense = _dense_conv(ops16, tmp_path, case, c, epi, {})
            _conv_view(ops16, tmp_path, case, c, epi, (off, ld, 0, 64, 0, 0), {}, f"bf16 conv {case} cut={cut} back={back} epilogue={epi}", BF16_BAR, dense)
    cx, cskip = cut
    cin = cskip if back else cx
    for k, stride in ((1, 1), (3, 2)) if cin % 64 == 0 else ():          # the 1x1 skip convolution and the stride-2 down convolution read the cut (bf16 kernels: Cin % 64 == 0)
        case = (1, cin, 10, 8, 64, k, stride, 0)
        c = _conv_case(case, "bf16")
        dense = _dense_conv(ops16, tmp_path, case, c, False, {})
        _conv_view(ops16, tmp_path, case, c, False, (0, 64, cx if back else 0, cx + cskip, 0, 0), {}, f"bf16 conv {case} reading cut {cut} back={back}", BF16_BAR, dense)


@pytest.mark.parametrize("back", [0, 1])
@pytest.mark.parametrize("cut", MODEL_CUTS)
def test_conv_view_model_cuts_mxfp8(ops8, tmp_path, cut, back):
    """conv_fp8 writes the cut (with temb / resid), and Engine::quantize reads one (launch_quantize_bf16_fp8 with ldx = ctot)"""
    case, (off, ld) = _cut_case(*cut, back, 3)
    c = _conv_case(case, "mx")
    cin = case[1]
    for epi in (False, True):
        what = f"mxfp8 conv {case} cut={cut} back={back} epilogue={epi}"
        dense, dlines = _conv_view(ops8, tmp_path, case, c, epi, (0, case[4], 0, cin, 0, 0), {}, what + " (dense strides)", BF16_BAR)
        assert " fp8 " in dlines[0], dlines
        _conv_view(ops8, tmp_path, case, c, epi, (off, ld, 64, 64 + cin + 32, 0, 0), {}, what, BF16_BAR, (dense, dlines))
    cx, cskip = cut
    cin = cskip if back else cx
    case = (1, cin, 9, 7, 64, 3, 1, 0)
    c = _conv_case(case, "mx")
    dense = _conv_view(ops8, tmp_path, case, c, False, (0, 64, 0, cin, 0, 0), {}, f"mxfp8 conv {case} (dense strides)", BF16_BAR)
    _conv_view(ops8, tmp_path, case, c, False, (0, 64, cx if back else 0, cx + cskip, 0, 0), {}, f"mxfp8 conv {case} quantising cut {cut} back={back}", BF16_BAR, dense)


# ---- 4. bf16: one-tile kernels 0-9, large tiles 100-103 x resid_acc x split-K (16-byte reduce forms), kernel-row tiles, conv_in's route ------------------------------
BF16_CASES = [(2, 64, 23, 19, 200, 3, 1, 0), (8, 128, 8, 8, 328, 3, 1, 0), (3, 64, 20, 18, 320, 3, 2, 0), (2, 128, 9, 11, 320, 3, 1, 1), (4, 192, 12, 13, 200, 1, 1, 0)]
# (out_off, pad behind, in_off, pad behind): multiples of 32, of 8 but not 32; the third has ldc % 8 == 4 -- set_resid_acc and vec_ok step down, the base stays on 16 bytes
BF16_VIEWS = [(0, 320, 0, 64), (320, 0, 64, 0), (8, 16, 8, 8), (8, 4, 0, 8), (0, 2, 8, 0)]


@pytest.mark.parametrize("case", BF16_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("ra", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", [100, 101, 102, 103])
def test_conv_view_bf16_large_tiles(ops16, tmp_path, tile, ra, splitk, case):
    n, cin, h, w, cout, k, stride, ups = case
    c = _conv_case(case, "bf16")
    opts = dict(gemm_tile=tile, splitk=splitk, resid_acc=ra)
    dense = _dense_conv(ops16, tmp_path, case, c, True, opts)
    _took(dense[1], f"dense {case} tile={tile}", tile, _splits(case, splitk, 64))
    for vi, (oo, opad, io, ipad) in enumerate(BF16_VIEWS):
        if (vi + tile + ra + splitk) % 2 and vi < 3:
            continue
        ld = oo + cout + opad
        what = f"bf16 conv {case} tile={tile} splitk={splitk} resid_acc={ra} view={(oo, ld, io, io + cin + ipad)}"
        _conv_view(ops16, tmp_path, case, c, True, (oo, ld, io, io + cin + ipad, 0, 0), opts, what, BF16_BAR, dense, _acc_gate(ld))


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("tile", list(range(10)))
def test_conv_view_bf16_small_tiles(ops16, tmp_path, tile, splitk):
    for case in [(3, 128, 9, 7, 200, 3, 1, 0), (1, 64, 12, 10, 72, 1, 1, 0)]:
        n, cin, h, w, cout, k, stride, ups = case
        c = _conv_case(case, "bf16")
        opts = dict(gemm_tile=tile, splitk=splitk)
        for epi in (False, True):
            dense = _dense_conv(ops16, tmp_path, case, c, epi, opts)
            _took(dense[1], f"dense {case} tile={tile}", tile, _splits(case, splitk, 64))
            for oo, opad, io, ipad in BF16_VIEWS:
                ld = oo + cout + opad
                what = f"bf16 conv {case} tile={tile} splitk={splitk} epilogue={epi} view={(oo, ld, io, io + cin + ipad)}"
                _conv_view(ops16, tmp_path, case, c, epi, (oo, ld, io, io + cin + ipad, 0, 0), opts, what, BF16_BAR, dense, _acc_gate(ld))


# 3x3 / stride 1, widths 16 ... 64, pixel counts that are multiples of the 256-row tile, k slices of whole kernel rows (TCASES of test_bf16_gpu.py): the layers tiles 104 / 105 accept
KROW_CASES = [(2, 128, 16, 16, 320, 3, 1, 0), (1, 64, 32, 32, 256, 3, 1, 0), (3, 192, 16, 16, 328, 3, 1, 0)]


@pytest.mark.parametrize("case", KROW_CASES)
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("tile", [104, 105])
def test_conv_view_bf16_kernel_row_tiles(ops16, tmp_path, tile, ra, case):
    """k_gemm_bf16t.hip stages an image row band of the SLICE (a_ld = the parent's width) once for its three taps"""
    n, cin, h, w, cout, k, stride, ups = case
    c = _conv_case(case, "bf16")
    opts = dict(gemm_tile=tile, splitk=1, resid_acc=ra)
    dense = _dense_conv(ops16, tmp_path, case, c, True, opts)
    _took(dense[1], f"dense {case}", tile, 1)
    for oo, opad, io, ipad in BF16_VIEWS[:4]:
        ld = oo + cout + opad
        _conv_view(ops16, tmp_path, case, c, True, (oo, ld, io, io + cin + ipad, 0, 0), opts, f"bf16 conv {case} tile={tile} resid_acc={ra} view={(oo, ld, io)}", BF16_BAR,
                   dense, _acc_gate(ld))


@pytest.mark.parametrize("tile", [100, 101, 102])
def test_conv_view_bf16_persistent_and_direct_epilogue(ops16, tmp_path, tile):
    """more tiles than the chip has CUs: the persistent tile loop, staggered DMA and general-epilogue variants (gemm_bf16x_variant 1, 4, 5, 8, 13) write the same slice
    bit for bit as one tile per workgroup, and none touches the neighbours"""
    case = (4, 64, 136, 136, 64, 1, 1, 0)
    n, cin, h, w, cout = case[:5]
    g = np.random.default_rng(7100 + tile)
    x = bf16_round(g.standard_normal((n, cin, h, w)))
    wt = bf16_round(g.standard_normal((cout, cin, 1, 1)) / math.sqrt(cin))
    b = g.standard_normal(cout).astype(np.float32)
    resid = bf16_round(g.standard_normal((n, cout, h, w)))
    off, ld = 64, 160
    pre = _prefill(n * h * w, ld)
    outs = {}
    try:
        ops16.set_option("gemm_tile", tile)
        ops16.set_option("splitk", 1)
        for v in (0, 1, 4, 5, 8, 13):
            ops16.set_option("gemm_bf16x_variant", v)
            outs[v] = ops16.op_conv2d_view(x, wt, b, None, resid, parent=pre, out_off=off, in_ld=cin + 64, in_off=32)
        dense = ops16.op_conv2d_epilogue(x, wt, b, None, resid)
    finally:
        ops16.set_option("gemm_tile", "auto")
        ops16.set_option("splitk", 0)
        ops16.set_option("gemm_bf16x_variant", "default")
    for v, p in outs.items():
        _neighbours_intact(p, pre, off, cout, f"bf16 persistent tile={tile} variant={v}")
        assert np.array_equal(_bits(p), _bits(outs[0])), f"bf16 persistent tile={tile}: variant {v} differs from 0"
    y = _nchw(outs[0], off, cout, n, h, w)
    assert np.array_equal(_bits(y), _bits(dense)), f"bf16 persistent tile={tile}: the slice differs from the dense result"
    hw = h * w
    for s in range(n):
        rs = np.r_[0:48, hw // 2 - 40:hw // 2 + 40, hw - 48:hw]
        ref = x[s].reshape(cin, hw)[:, rs].T.astype(np.float64) @ wt.reshape(cout, cin).T.astype(np.float64) + b + resid[s].reshape(cout, hw)[:, rs].T
        _check(y[s].reshape(cout, hw)[:, rs].T, ref, f"bf16 persistent tile={tile} sample {s}", BF16_BAR)


@pytest.mark.parametrize("view", [(0, 320), (320, 0), (8, 16), (8, 4)])
def test_conv_in_view_bf16(ops16, tmp_path, view):
    """conv_in: Cin = 4, the fp32 kernel emitting bf16 (out_mode 2) writes the back slice of the first concat buffer"""
    case = (2, 4, 23, 19, 320, 3, 1, 0)
    c = _conv_case(case, "f32")
    oo, opad = view
    for tile in ("auto", 0, 3, 7):
        opts = dict(gemm_tile=tile)
        x, wt, b = c[:3]
        n, cin, h, w, cout = case[:5]
        pre = _prefill(n * h * w, oo + cout + opad)
        got, lines = _run(ops16, tmp_path, lambda: ops16.op_conv2d_view(x, wt, b, parent=pre, out_off=oo, in_ld=8, in_off=4), **opts)
        what = f"conv_in bf16 tile={tile} view={view}"
        _neighbours_intact(got, pre, oo, cout, what)
        y = _nchw(got, oo, cout, n, h, w)
        _check(y, _ref(c[5], b), what, BF16_BAR)
        bd, dlines = _run(ops16, tmp_path, lambda: ops16.op_conv2d(x, wt, b), **opts)
        assert lines == dlines, (lines, dlines)
        assert np.array_equal(_bits(y), _bits(bd)), f"{what}: differs from the dense result"


# ---- 5. MXFP8: conv_fp8 into a slice, forced tiles and split-K; gemm_fp8; the refusal of a stride off 8 ------------------------------------------------------------------
FP8_CASES = [(2, 320, 16, 16, 320, 3, 1, 0), (1, 256, 24, 40, 200, 3, 1, 0), (3, 64, 5, 7, 96, 3, 1, 0)]
FP8_VIEWS = [(0, 320, 0, 64), (320, 0, 64, 0), (8, 16, 8, 8), (40, 8, 32, 0)]


@pytest.mark.parametrize("case", FP8_CASES)
@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("ra", [0, 3])
@pytest.mark.parametrize("tile", ["auto", 0, 1, 2])
def test_conv_view_mxfp8(ops8, tmp_path, tile, ra, splitk, case):
    n, cin, h, w, cout, k, stride, ups = case
    c = _conv_case(case, "mx")
    opts = dict(fp8_tile=tile, splitk=splitk, resid_acc=ra)
    for epi in (False, True):
        dense = _conv_view(ops8, tmp_path, case, c, epi, (0, cout, 0, cin, 0, 0), opts, f"mxfp8 conv {case} (dense strides)", BF16_BAR)
        assert " fp8 " in dense[1][0] and f" splits={splitk} " in dense[1][0], dense[1]
        for oo, opad, io, ipad in FP8_VIEWS:
            ld = oo + cout + opad
            what = f"mxfp8 conv {case} fp8_tile={tile} splitk={splitk} resid_acc={ra} epilogue={epi} view={(oo, ld, io, io + cin + ipad)}"
            _conv_view(ops8, tmp_path, case, c, epi, (oo, ld, io, io + cin + ipad, 0, 0), opts, what, BF16_BAR, dense)


@pytest.mark.parametrize("shape", [(300, 320, 200), (1024, 1280, 320), (77, 64, 160)])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "mx"])
def test_linear_view(ops32, ops16, ops8, tmp_path, fmt, shape):
    """gemm / gemm_fp8 with ldc > N: the attention and feed-forward output projections' form, written into a slice with a residual"""
    rows, cin, cout = shape
    sd, bar = {"f32": (ops32, FP32_BAR), "bf16": (ops16, BF16_BAR), "mx": (ops8, BF16_BAR)}[fmt]
    g = np.random.default_rng(zlib.crc32(repr((shape, fmt)).encode()))
    x = g.standard_normal((rows, cin)).astype(np.float32)
    wt = (g.standard_normal((cin, cout)) / math.sqrt(cin)).astype(np.float32)
    resid = g.standard_normal((rows, cout)).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    if fmt == "bf16":
        x, wt, resid = bf16_round(x), bf16_round(wt), bf16_round(resid)
    elif fmt == "mx":
        x = MX.mx_quantize(_t(x) * 1.5, 1).numpy().astype(np.float32)
        wt = MX.mx_quantize(_t(wt), 0).numpy().astype(np.float32)
        resid = bf16_round(resid)
    ref = O.linear(_t(x), _t(wt), _t(b)).numpy() + resid
    base = dict(fp8_ops=1) if fmt == "mx" else {}
    tiles = {"f32": ["auto", 3, 101, 203, 304], "bf16": ["auto", 3, 100, 102], "mx": ["auto", 0, 2]}[fmt]
    for tile in tiles:
        for splitk in (1, 3):
            opts = dict(base, splitk=splitk, **({"fp8_tile": tile} if fmt == "mx" else {"gemm_tile": tile}))
            dense, dlines = _run(sd, tmp_path, lambda: sd.op_linear_epilogue(x, wt, b, resid, resid_ld=cout + 8), **opts)
            views = [(0, 320), (320, 0), (8, 16), (32, 32)] + ([(4, 8), (0, 2)] if fmt == "f32" else [(8, 4)] if fmt == "bf16" else [])
            for oo, opad in views:
                ld = oo + cout + opad
                pre = _prefill(rows, ld)
                what = f"{fmt} linear {shape} tile={tile} splitk={splitk} view={(oo, ld)}"
                got, lines = _run(sd, tmp_path, lambda: sd.op_linear_view(x, wt, b, resid, resid_ld=cout + 8, parent=pre, out_off=oo), **opts)
                _neighbours_intact(got, pre, oo, cout, what)
                y = got[:, oo:oo + cout]
                _check(y, ref, what, bar)
                if lines == dlines:
                    assert np.array_equal(_bits(y), _bits(dense)), f"{what}: same launch record as the dense call but different bits"
                else:
                    assert _acc_gate(ld)(lines, dlines), f"{what}: {lines} vs {dlines}"


def test_mxfp8_refuses_a_stride_off_eight(ops8, tmp_path):
    """k_fp8.hip has the 16-byte epilogue only: ldc % 8 != 0 is an error code, and nothing of the parent is written"""
    from stable_diffusion_burn_amd import SdmiError
    case = (1, 64, 12, 10, 96, 3, 1, 0)
    x, wt, b, temb, resid, conv = _conv_case(case, "mx")
    pre = _prefill(120, 8 + 96 + 4)
    with pytest.raises(SdmiError) as ei:
        ops8.op_conv2d_view(x, wt, b, parent=pre, out_off=8)
    assert ei.value.status < 0 and np.array_equal(_bits(ei.value.parent), _bits(pre)), "conv_fp8 wrote part of a parent it refused"
    g = np.random.default_rng(3)
    xl, wl = g.standard_normal((77, 64)).astype(np.float32), (g.standard_normal((64, 160)) / 8).astype(np.float32)
    pre = _prefill(77, 8 + 160 + 4)
    try:
        ops8.set_option("fp8_ops", 1)
        with pytest.raises(SdmiError) as ei:
            ops8.op_linear_view(xl, wl, None, parent=pre, out_off=8)
    finally:
        ops8.set_option("fp8_ops", 0)
    assert ei.value.status < 0 and np.array_equal(_bits(ei.value.parent), _bits(pre)), "gemm_fp8 wrote part of a parent it refused"
    # the same parents one column wider are served
    pre = _prefill(120, 8 + 96 + 8)
    got = ops8.op_conv2d_view(x, wt, b, parent=pre, out_off=8)
    _neighbours_intact(got, pre, 8, 96, "mxfp8 conv next to the refused stride")
    _check(_nchw(got, 8, 96, 1, 12, 10), _ref(conv, b), "mxfp8 conv next to the refused stride", BF16_BAR)


# ---- 6. GroupNorm reading a slice: fp32, planes, bf16, MXFP8 output ------------------------------------------------------------------------------------------------------------
# (n, c, h, w, in_off, in_ld): the model's skips at one chunk and many chunks per sample, then the small shapes of the dense tests
GN_CASES = [(1, 320, 64, 64, 320, 640), (2, 320, 64, 64, 0, 640), (1, 640, 32, 32, 640, 1280), (2, 640, 32, 32, 1280, 1920), (2, 320, 16, 16, 640, 960),
            (1, 1280, 8, 8, 1280, 2560), (1, 128, 32, 32, 32, 192), (1, 32, 4, 4, 8, 48), (2, 640, 1, 1, 160, 960), (1, 160, 16, 16, 160, 320)]
GN_FORMS = ["fp32", "planes", "bf16", "mxfp8"]


def _gn_engine(form, ops32, ops16, ops8):
    return {"fp32": (ops32, 0), "planes": (ops32, 1), "bf16": (ops16, 0), "mxfp8": (ops8, 2)}[form]


def _gn_settings(form):
    if form in ("fp32", "planes"):
        return [{}, {"gn32_min_wgs": 1, "gn32_stats_min_wgs": -1}, {"gn32_min_wgs": 1024, "gn32_stats_min_wgs": 512}]
    return [{}, {"gn_target_wgs": 64, "gn_unroll": 1}, {"gn_target_wgs": 2048, "gn_unroll": 4}]


def _gn_check(form, got, ref, what):
    if form == "mxfp8":          # the bars of test_group_norm_mxfp8_output
        assert np.isfinite(got).all(), f"{what}: non-finite output (a neighbour column read?)"
        want = MX.mx_quantize(torch.from_numpy(ref), 1).numpy()
        frac = (got == want).mean()
        assert frac > 0.995, f"{what}: only {100 * frac:.2f} % of the elements identical to the oracle quantiser"
        assert (np.abs(got - ref) <= 0.13 * np.abs(ref) + 2e-3).all(), what
    else:
        _check(got, ref, what, BF16_BAR if form == "bf16" else FP32_BAR)


@pytest.mark.parametrize("case", GN_CASES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("form", GN_FORMS)
def test_group_norm_view(ops32, ops16, ops8, tmp_path, form, silu, case):
    n, c, h, w, off, ld = case
    sd, fcode = _gn_engine(form, ops32, ops16, ops8)
    g = np.random.default_rng(c * 7 + h + off)
    x = (g.standard_normal((n, c, h, w)) * 1.7 + 0.9).astype(np.float32)
    if form in ("bf16", "mxfp8"):
        x = bf16_round(x)
    gamma = (1 + 0.1 * g.standard_normal(c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c)).astype(np.float32)
    ref = O.group_norm(_t(x), _t(gamma), _t(beta), 32, 1e-5)
    if silu:
        ref = O.silu(ref)
    ref = ref.numpy()
    for opts in _gn_settings(form):
        what = f"group_norm {form} {case} silu={silu} settings={opts}"
        got, _ = _run(sd, tmp_path, lambda: sd.op_group_norm_view(x, gamma, beta, 1e-5, silu, in_ld=ld, in_off=off, in_planes=3 if (form == "planes" and off % 32 == 0 and ld % 32 == 0) else 0,
                                                                  form=fcode), **opts)
        _gn_check(form, got, ref, what)
        # the same launch on a dense tensor: same values in the same order (the dense fp32 entry takes the plane-writing form under option gemm_planes, the default)
        dopts = dict(opts, gemm_planes=0) if form == "fp32" else opts
        dense, _ = _run(sd, tmp_path, lambda: (sd.op_group_norm_fp8 if form == "mxfp8" else sd.op_group_norm)(x, gamma, beta, 32, 1e-5, silu), **dopts)
        assert np.array_equal(_bits(got), _bits(dense)), f"{what}: differs from the dense launch"


@pytest.mark.parametrize("form", GN_FORMS)
@pytest.mark.parametrize("fill", [NAN, 7.0])
def test_group_norm_view_large_mean(ops32, ops16, ops8, form, fill):
    """|mean| >> std inside the slice, the neighbour columns at ANOTHER mean (7: finite, so a statistic that strays over the slice edge by a few channels is an error
    far above the bar, not only a NaN) or NaN"""
    sd, fcode = _gn_engine(form, ops32, ops16, ops8)
    n, c, h, w, off, ld = 2, 320, 32, 32, 320, 960
    mean, std = (30.0, 0.05) if form in ("fp32", "planes") else (30.0, 0.5)
    g = np.random.default_rng(5)
    x = (g.standard_normal((n, c, h, w)) * std + mean).astype(np.float32)
    x += (g.standard_normal((1, c, 1, 1)) * 3 * std).astype(np.float32)
    if form in ("bf16", "mxfp8"):
        x = bf16_round(x)
    gamma = (1 + 0.1 * g.standard_normal(c)).astype(np.float32)
    beta = (0.1 * g.standard_normal(c)).astype(np.float32)
    ref = O.group_norm(_t(x), _t(gamma), _t(beta), 32, 1e-5).numpy()
    got = sd.op_group_norm_view(x, gamma, beta, 1e-5, False, in_ld=ld, in_off=off, in_fill=fill, form=fcode)
    _gn_check(form, got, ref, f"group_norm {form} large mean, neighbours {fill}")
    front = sd.op_group_norm_view(x, gamma, beta, 1e-5, False, in_ld=ld, in_off=0, in_fill=fill, form=fcode)
    assert np.array_equal(_bits(got), _bits(front)), "the front and the back slice of the same values differ"


# ---- 7. a block boundary: two convolutions write the halves, GroupNorm reads the whole ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [(320, 320), (640, 320), (160, 160), (320, 160), (200, 120)])
@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_cat_chain(ops32, ops16, fmt, cut):
    sd, bar = (ops32, FP32_BAR) if fmt == "f32" else (ops16, BF16_BAR)
    cx, cskip = cut
    n, cin, h, w = 2, 64, 13, 11
    g = np.random.default_rng(cx * 3 + cskip)
    x = g.standard_normal((n, cin, h, w)).astype(np.float32)
    wx = (g.standard_normal((cx, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32)
    ws = (g.standard_normal((cskip, cin, 3, 3)) / math.sqrt(cin * 9)).astype(np.float32)
    if fmt == "bf16":
        x, wx, ws = bf16_round(x), bf16_round(wx), bf16_round(ws)
    bx, bs = g.standard_normal(cx).astype(np.float32), (g.standard_normal(cskip) + 2.0).astype(np.float32)
    gamma = (1 + 0.1 * g.standard_normal(cx + cskip)).astype(np.float32)
    beta = (0.1 * g.standard_normal(cx + cskip)).astype(np.float32)
    views = sd.op_cat_chain(x, wx, bx, ws, bs, gamma, beta, silu=True, dense=False)
    dense = sd.op_cat_chain(x, wx, bx, ws, bs, gamma, beta, silu=True, dense=True)
    assert np.array_equal(_bits(views), _bits(dense)), f"cat chain {fmt} {cut}: slices and concat copy differ"
    if fmt == "f32":
        ya, yb = O.conv2d(_t(x), (_t(wx), _t(bx)), padding=1), O.conv2d(_t(x), (_t(ws), _t(bs)), padding=1)
    else:
        # the halves are STORED as bf16 between the two operators: the GroupNorm bar is held against the oracle on the halves as the same two launches store them
        # (each within the convolution's own bar of its oracle)
        ya, yb = _t(sd.op_conv2d(x, wx, bx)), _t(sd.op_conv2d(x, ws, bs))
        _check(ya.numpy(), O.conv2d(_t(x), (_t(wx), _t(bx)), padding=1).numpy(), f"cat chain {fmt} {cut}: front half", bar)
        _check(yb.numpy(), O.conv2d(_t(x), (_t(ws), _t(bs)), padding=1).numpy(), f"cat chain {fmt} {cut}: back half", bar)
    ref = O.silu(O.group_norm(torch.cat([ya, yb], dim=1), _t(gamma), _t(beta), 32, 1e-5)).numpy()
    _check(views, ref, f"cat chain {fmt} {cut}", bar)


# ---- 8. arguments ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_views_are_refused_before_anything_runs(ops32, ops16):
    from stable_diffusion_burn_amd import SdmiError
    case = (1, 64, 6, 5, 96, 1, 1, 0)
    x, wt, b = _conv_case(case, "f32")[:3]
    pre = _prefill(30, 160)
    for sd in (ops32, ops16):
        for kw in (dict(out_off=-32), dict(out_off=96), dict(out_off=0, in_ld=32), dict(out_off=0, in_ld=96, in_off=64), dict(out_off=0, in_ld=96, in_off=-32)):
            with pytest.raises(SdmiError) as ei:
                sd.op_conv2d_view(x, wt, b, parent=pre, **kw)
            assert "view" in str(ei.value), ei.value
            assert np.array_equal(_bits(ei.value.parent), _bits(pre))
            bad_status = ei.value.status
        with pytest.raises(SdmiError) as ei:
            sd.op_conv2d_view(x, wt, b, parent=_prefill(30, 64), out_off=0)      # ld < c
        assert ei.value.status == bad_status
        with pytest.raises(SdmiError):
            sd.op_group_norm_view(np.zeros((1, 64, 4, 4), np.float32), np.ones(64, np.float32), np.zeros(64, np.float32), in_ld=96, in_off=64)
        with pytest.raises(SdmiError):
            sd.op_linear_view(np.zeros((30, 64), np.float32), np.zeros((64, 96), np.float32), parent=pre, out_off=80)
    # what Engine::slice refuses comes back as ITS error (not a fault): planes cut off a multiple of 32 channels, a base off 16 bytes
    with pytest.raises(SdmiError) as ei:
        ops32.op_conv2d_view(x, wt, b, parent=pre, out_off=16, out_planes=3)
    assert "slice" in str(ei.value) and ei.value.status != bad_status and np.array_equal(_bits(ei.value.parent), _bits(pre))
    with pytest.raises(SdmiError) as ei:
        ops32.op_conv2d_view(x, wt, b, parent=pre, out_off=2)
    assert "slice" in str(ei.value) and np.array_equal(_bits(ei.value.parent), _bits(pre))
    x16, wt16 = bf16_round(x), bf16_round(wt)
    with pytest.raises(SdmiError) as ei:
        ops16.op_conv2d_view(x16, wt16, b, parent=pre, out_off=4)               # 8 bytes into a bf16 row: the 16-byte stores of vec_ok would be misaligned
    assert "slice" in str(ei.value) and np.array_equal(_bits(ei.value.parent), _bits(pre))
    with pytest.raises(SdmiError) as ei:
        ops16.op_group_norm_view(np.zeros((1, 64, 4, 4), np.float32), np.ones(64, np.float32), np.zeros(64, np.float32), in_ld=96, in_off=4)
    assert "slice" in str(ei.value)
