"""fp32 up-convolutions as four folded 2x2 phase convolutions in one plane launch (csrc/kernels.hpp ConvGemm::phases; option ups_phase), precision 0, through the
operator entry points: ups_phase = 1 (wherever supported) against ups_phase = 0 (the K = 9 Cin launch over the 4 x larger grid).

Every case holds
  * both arms to the fp64 oracle conv3x3(upsample2x(x)) at the operator bar 2e-5 max(1, |ref|);
  * the two arms to each other within two bars at every element;
  * the phase arm run twice to the same bits;
  * the " phase " token in the phase arm's dump_choices record, and its absence in the other arm's.
The shapes are the smallest that reach each way of going wrong (named at each case).  The half-width model runs one UNet forward and one decode under both arms at
the bars of tests/test_model_gpu.py, and again after a LoRA scale change on an upsample convolution: a stale fold must not run, and the fold is re-derived."""
import math
import zlib

import numpy as np
import pytest
import torch

import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, SdmiError, StableDiffusion
from stable_diffusion_burn_amd import synthetic as syn
from test_model_gpu import _assert_close

pytestmark = pytest.mark.gpu

FP32_BAR = 2e-5
_RESTORE = {"ups_phase": "default", "gemm_tile": "auto", "splitk": 0}


@pytest.fixture(scope="module")
def ops():
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=0))
    yield sd
    sd.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_CASES = {}


def _case(case):
    """x, weight, bias and the fp64 reference of one shape (n, cin, h, w, cout), computed once"""
    if case not in _CASES:
        n, cin, h, w, cout = case
        g = np.random.default_rng(zlib.crc32(repr((case, "ups_phase_gpu")).encode()))
        x = g.standard_normal((n, cin, h, w)).astype(np.float32)
        wt = (g.standard_normal((cout, cin, 3, 3)) / math.sqrt(9 * cin)).astype(np.float32)
        b = g.standard_normal(cout).astype(np.float32)
        t = lambda a: torch.from_numpy(a).double()
        ref = O.conv2d(O.upsample2x(t(x)), (t(wt), t(b)), stride=1, padding=1).numpy()
        ref.setflags(write=False)
        _CASES[case] = (x, wt, b, ref)
    return _CASES[case]


def _run(sd, tmp_path, fn, **opts):
    """fn() under the given options (restored afterwards) -> (result, its dump_choices lines)"""
    path = tmp_path / "choices.txt"
    try:
        for k, v in opts.items():
            sd.set_option(k, v)
        sd.set_option("record_shapes", 1)
        try:
            out = fn()
        finally:
            sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
        for k in opts:
            sd.set_option(k, _RESTORE[k])
    return out, path.read_text().splitlines()


def _within(got, ref, bars, what, oracle=None):
    """max |got - ref| <= bars x the operator bar, which is scaled by the oracle (ref itself unless given)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = np.abs(got - ref).max()
    bound = bars * FP32_BAR * max(1.0, np.abs(ref if oracle is None else oracle).max())
    print(f"{what}: max|d| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max|d|={err:.3e} > {bound:.3e}"


def _both_arms(sd, tmp_path, case, what, **opts):
    """the checks every case makes; returns the phase arm's record"""
    x, wt, b, ref = _case(case)
    call = lambda: sd.op_conv2d_epilogue(x, wt, b, upsample2x=True)
    ph, ph_lines = _run(sd, tmp_path, call, ups_phase=1, **opts)
    ph2, _ = _run(sd, tmp_path, call, ups_phase=1, **opts)
    td, td_lines = _run(sd, tmp_path, call, ups_phase=0, **opts)
    assert len(ph_lines) == 1 and " phase " in ph_lines[0], f"{what}: no phase launch recorded: {ph_lines}"
    assert len(td_lines) == 1 and " phase " not in td_lines[0], f"{what}: ups_phase=0 recorded {td_lines}"
    n, cin, h, w, cout = case
    head = f"{n * 4 * h * w},{cout},{9 * cin} k3 s1 u1 W{w} phase cfg="
    assert ph_lines[0].startswith(head) and " splits=" in ph_lines[0], f"{what}: the record is not under the layer's head {head!r}: {ph_lines[0]}"
    _within(ph, ref, 1, f"{what}, phases [{ph_lines[0]}]")
    _within(td, ref, 1, f"{what}, today's launch [{td_lines[0]}]")
    _within(ph, td, 2, f"{what}, the two arms", oracle=ref)
    assert np.array_equal(_bits(ph), _bits(ph2)), f"{what}: two runs of the phase arm differ"
    return ph_lines[0]


def test_less_than_one_tile_per_phase(ops, tmp_path):
    """M = 70 rows per phase: masked rows in every phase's only tile, an N tail (48), every border, fragment groups that straddle scanlines (7 wide) and samples"""
    _both_arms(ops, tmp_path, (2, 32, 5, 7, 48), "2x32x5x7 -> 48")


def test_one_source_pixel(ops, tmp_path):
    """all taps but one of every phase are padding"""
    _both_arms(ops, tmp_path, (1, 64, 1, 1, 32), "1x64x1x1 -> 32")


@pytest.mark.parametrize("splitk", [1, 2, 3])
def test_split_k_and_the_reduce_row_map(ops, tmp_path, splitk):
    """two 256-row tiles per phase (tile 301); 8 k tiles, split raggedly by 3: the slabs are [splits][4][M][N] and the reduce writes through the row map"""
    ln = _both_arms(ops, tmp_path, (2, 64, 16, 16, 64), f"2x64x16x16 -> 64 splitk={splitk}", gemm_tile=301, splitk=splitk)
    assert " cfg=301 " in ln and f" splits={splitk} " in ln, ln


@pytest.mark.parametrize("tile", list(range(300, 309)))
def test_every_plane_tile(ops, tmp_path, tile):
    """M = 180 rows per phase, N = 80: interior and edge tiles of every plane tile shape (64 ... 256 rows, 64 ... 320 columns)"""
    ln = _both_arms(ops, tmp_path, (1, 96, 9, 20, 80), f"1x96x9x20 -> 80 tile={tile}", gemm_tile=tile)
    assert f" cfg={tile} " in ln, ln


@pytest.mark.parametrize("mode", [1, 2])
def test_view_into_a_channel_slice(ops, tmp_path, mode):
    """planes in (a slice of a wider parent), fp32 and planes out into a channel slice at a non-zero offset of a wider parent: ldc / ldc3 views.  The plane output
    joined back equals the fp32 output bit for bit and the parent is untouched outside the slice.  mode 2: the default takes this launch by itself (the activations
    arrive as planes, 512 rows per phase, automatic tile)."""
    case = (2, 64, 16, 16, 64)
    x, wt, b, ref = _case(case)
    n, cin, h, w, cout = case
    out_off, out_ld, in_off, in_ld = 32, 160, 32, 128
    rows = n * 4 * h * w
    r = np.arange(rows, dtype=np.int64)[:, None]
    j = np.arange(out_ld, dtype=np.int64)[None, :]
    pre = (((r * 131 + j * 7) % 251 - 125) / 4.0).astype(np.float32)      # exact in bf16 and in the three-plane split
    call = lambda: ops.op_conv2d_view(x, wt, b, upsample2x=True, parent=pre, out_off=out_off, in_ld=in_ld, in_off=in_off, in_planes=3, out_planes=3)
    (pf, pp), lines = _run(ops, tmp_path, call, ups_phase=mode)
    (tf, tp), tlines = _run(ops, tmp_path, call, ups_phase=0)
    assert len(lines) == 1 and " phase " in lines[0], lines
    assert len(tlines) == 1 and " phase " not in tlines[0], tlines
    keep = np.ones(out_ld, bool)
    keep[out_off:out_off + cout] = False
    for what, parent in (("fp32 copy", pf), ("plane copy", pp)):
        assert np.array_equal(_bits(parent)[:, keep], _bits(pre)[:, keep]), f"view, {what}: the parent changed outside the slice [{out_off}, {out_off + cout})"
    assert np.array_equal(_bits(pf), _bits(pp)), "view: the plane output joined back differs from the fp32 output"
    nchw = lambda parent: np.ascontiguousarray(parent[:, out_off:out_off + cout].reshape(n, 2 * h, 2 * w, cout).transpose(0, 3, 1, 2))
    _within(nchw(pf), ref, 1, f"view, phases [{lines[0]}]")
    _within(nchw(tf), ref, 1, f"view, today's launch [{tlines[0]}]")
    _within(nchw(pf), nchw(tf), 2, "view, the two arms", oracle=ref)
    (pf2, _), _ = _run(ops, tmp_path, call, ups_phase=mode)
    assert np.array_equal(_bits(pf), _bits(pf2)), "view: two runs of the phase arm differ"


def test_phases_with_a_residual_are_refused(ops, tmp_path):
    """a phase launch carries the bias only: the forced arm with a residual is an error, and nothing is launched"""
    case = (2, 64, 16, 16, 64)
    x, wt, b, ref = _case(case)
    resid = np.zeros(ref.shape, np.float32)
    with pytest.raises(SdmiError):
        _run(ops, tmp_path, lambda: ops.op_conv2d_epilogue(x, wt, b, None, resid, upsample2x=True), ups_phase=1)
    assert (tmp_path / "choices.txt").read_text().split() == [], "a launch was recorded"
    # the default declines instead: today's launch adds the residual
    got, lines = _run(ops, tmp_path, lambda: ops.op_conv2d_epilogue(x, wt, b, None, resid, upsample2x=True), ups_phase=2)
    assert len(lines) == 1 and " phase " not in lines[0], lines
    _within(got, ref, 1, "residual, default plan")


# ---- the half-width model ------------------------------------------------------------------------------------------------------------------------------------
UP1, UP2 = "unet/output_blocks/rtu1/upsample/conv/weight", "unet/output_blocks/rtu2/upsample/conv/weight"


def test_half_width_model_and_a_lora_scale_change(synth, tiny_dims, tmp_path):
    d = tiny_dims
    c = d.model_channels
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch))
    try:
        sd.set_option("keep_masters", 1)
        sd.load_weights(synth, clip=False, vae_encoder=False)
        lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)])
        ctx = np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)])
        z = (np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(2)]) * 3.0).astype(np.float32)
        tl, tc, tz = torch.from_numpy(lat), torch.from_numpy(ctx), torch.from_numpy(z)
        a_cp = syn.alphas_cumprod()

        def pair(provider, what, decode):
            o32, o64 = (O.StableDiffusionOracle(provider, a_cp, d, dt) for dt in (torch.float32, torch.float64))
            r32, r64 = (o.unet.forward(tl, 500, tc).numpy() for o in (o32, o64))
            outs = {}
            for mode in (1, 0):
                got, lines = _run(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), ups_phase=mode)
                n_phase = sum(" phase " in ln for ln in lines)
                assert n_phase == (3 if mode else 0), f"{what} ups_phase={mode}: {n_phase} phase records among the UNet's launches (a stale or missing fold?)"
                e64, e32 = _assert_close(got, r32, r64, f"{what} unet_forward ups_phase={mode}", atol=1e-4)
                print(f"{what} unet ups_phase={mode}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
                outs[mode] = got
            if decode:
                d32, d64 = (o.decoder.decode_latent(tz).numpy() for o in (o32, o64))
                for mode in (1, 0):
                    got, lines = _run(sd, tmp_path, lambda: sd.autoencoder.decode_latent(z), ups_phase=mode)
                    assert sum(" phase " in ln for ln in lines) == (3 if mode else 0), f"{what} decode ups_phase={mode}: {lines}"
                    e64, e32 = _assert_close(got, d32, d64, f"{what} decode_latent ups_phase={mode}")
                    print(f"{what} decode ups_phase={mode}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
            return outs

        base = pair(synth, "base", True)
        ad = L.make_adapter({UP1: ((4 * c, 4 * c, 3, 3), 4), UP2: ((2 * c, 2 * c, 3, 3), 4)}, 23, rel=0.5)
        a = sd.lora_attach(ad, scale=1.0)
        try:
            a.set_scale(0.6)
            moved = pair(L.LoraProvider(synth, [(ad, 0.6)]), "adapted", False)
        finally:
            a.detach()
        # the adapter is visible far above the bar, so a stale fold (the un-adapted weights) could not have passed the oracle of the adapted model
        delta = float(np.abs(moved[1] - base[1]).max())
        print(f"max |adapted - base| (phase arm) = {delta:.3e}")
        assert delta > 20 * 1e-4
        back, _ = _run(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), ups_phase=1)
        assert np.array_equal(_bits(back), _bits(base[1])), "detach did not give the loaded model's phase launch back bit for bit"
    finally:
        sd.close()
