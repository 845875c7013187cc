"""ControlNet for SD v1 on the GPU (include/sdmi.h "ControlNet"), through the C ABI, against the CPU restatement in
tests/controlnet_ref.py.  Every bar is a neighbouring module's: test_img2img_gpu (fp32: the GPU's error against the fp64 oracle held against the fp32 oracle's
own), test_views_gpu (operator level), test_bf16_gpu / test_fp8_gpu (relative RMS at precision 1 / 2), test_scratch_fill_gpu (the pool_fill sweep)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import controlnet_ref as CR
import img2img_ref as R
import sampler_ref as SR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd import weights as W
from test_bf16_gpu import BAR_LATENT, BAR_UNET
from test_hires_gpu import BF16_DIMS
from test_img2img_gpu import _assert_close
from test_scratch_fill_gpu import _fills, _sweep
from test_views_gpu import BF16_BAR, FP32_BAR, _check

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_WEIGHTS, SDMI_ERR_UNSUPPORTED, SDMI_ERR_STATE = -1, -3, -5, -6
BAR_UNET_FP8 = 1.28e-1     # tests/test_fp8_gpu.py test_unet_forward_mxfp8, fp8_linear = 0: rel-RMS of a UNet forward against the exact fp64 oracle
N, T = 2, 7
ZERO_NAMES = [f"controlnet/zero_convs/{j}" for j in range(12)] + ["controlnet/middle_block_out"]


def _make(d, precision=0, control=3, h=None, w=None, **kw):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    return StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, h or d.latent_h, w or d.latent_w, d.vae_ch, precision=precision,
                                       control_hint_ch=control, **kw))


@pytest.fixture(scope="module")
def sdc(tiny_dims, synth):
    sd = _make(tiny_dims)
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture
def sd(sdc, tiny_dims):
    """the module's fp32 context; whatever a test sets, the next one finds no control, the default sampler and the configured size"""
    yield sdc
    sdc.set_control(None)
    sdc.set_sampler(None)
    sdc.set_latent_size(tiny_dims.latent_h, tiny_dims.latent_w)


@pytest.fixture(scope="module", params=[1, 2])
def sd_lowp(request, synth):
    sd = _make(BF16_DIMS, request.param)
    sd.load_weights(synth, clip=False)
    if request.param == 2:
        sd.set_option("fp8_min_rows", 1)     # 16 x 16 latents have few rows per GEMM: the MXFP8 path anyway (tests/test_fp8_gpu.py)
    yield sd, request.param
    sd.set_control(None)
    sd.close()


def _hints(d, n=N, seed=0, h=None, w=None):
    """n different random u8 hints of 8h x 8w with the values 0 and 255 present"""
    g = np.random.default_rng(900 + seed)
    hint = g.integers(0, 256, (n, 8 * (h or d.latent_h), 8 * (w or d.latent_w), 3), dtype=np.uint8)
    hint[1::2] //= 4                 # every second hint is a dark picture: two hints of a call differ in more than their noise
    hint[:, 3:9, 5:40] = 0
    hint[:, 20:31, 7:60] = 255
    return hint


def _inputs(d, n=N, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(3, d.ctx_dim)
    lat = np.stack([syn.initial_latent(40 + seed + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, lat


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def _status(fn):
    from stable_diffusion_burn_amd import SdmiError
    try:
        fn()
    except SdmiError as e:
        return e.status, str(e)
    return 0, ""


# ---- 1. the fp32 convolution route the hint convolutions run on, at every precision ------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1])
def ops_f32(request):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=request.param))
    sd.set_option("op_f32", 1)
    yield sd, request.param
    sd.close()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("cin", [16, 32, 96, 256])
def test_hint_convolution_route(ops_f32, cin, stride):
    sd, precision = ops_f32
    g = np.random.default_rng(cin * 10 + stride)
    cout = {16: 32, 32: 96, 96: 256, 256: 160}[cin]
    x = g.standard_normal((2, cin, 16, 16)).astype(np.float32)
    w = (g.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = g.standard_normal(cout).astype(np.float32)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=stride, padding=1).numpy()
    _check(sd.op_conv2d(x, w, b, stride=stride), ref, f"fp32-route conv cin={cin} stride={stride} in a precision-{precision} engine", FP32_BAR)


# ---- 2. the hint embedding ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(16, 16), (8, 24)])
def test_hint_embedding(sd, synth, tiny_dims, h, w):
    d = tiny_dims
    hint = _hints(d, h=h, w=w, seed=h)
    assert hint.min() == 0 and hint.max() == 255
    sd.set_latent_size(h, w)
    got = sd.control_hint_embed(hint)
    refs = [CR.ControlNetOracle(synth, d, dt).hint_embed(CR.hint01(hint)).numpy() for dt in (torch.float32, torch.float64)]
    assert got.shape == (N, d.model_channels, h, w)
    e64, e32 = _assert_close(got, refs[0], refs[1], f"hint embedding {h}x{w}")
    print(f"hint embedding {h}x{w}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


def test_hint_embedding_is_fp32_at_every_precision(sd_lowp):
    sd, precision = sd_lowp
    hint = _hints(BF16_DIMS, seed=3)
    ref = CR.ControlNetOracle(syn.SyntheticWeights(), BF16_DIMS, torch.float64).hint_embed(CR.hint01(hint)).numpy()
    _check(sd.control_hint_embed(hint), ref, f"hint embedding at precision {precision}", FP32_BAR)


# ---- 3. the 13 residuals -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _residuals_ref(wide: bool, dtype, t):
    d = BF16_DIMS if wide else O.Dims(160, 4, 64, 16, 16, 32)
    ctx, _, lat = _inputs(d)
    r = CR.ControlNetOracle(syn.SyntheticWeights(cache=True), d, dtype).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx), CR.hint01(_hints(d)))
    return [v.numpy() for v in r]


@pytest.mark.parametrize("t", [999, 1])
def test_residuals_fp32(sd, tiny_dims, t):
    d = tiny_dims
    assert d == O.Dims(160, 4, 64, 16, 16, 32)
    ctx, _, lat = _inputs(d)
    sd.set_control(_hints(d), strength=0.0)     # the entry ignores the strength
    got = sd.control_residuals(lat, t, ctx)
    r32, r64 = _residuals_ref(False, torch.float32, t), _residuals_ref(False, torch.float64, t)
    assert len(got) == 13
    for j in range(13):
        e64, e32 = _assert_close(got[j], r32[j], r64[j], f"residual {j} t={t}")
        print(f"residual {j} t={t} {got[j].shape}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


@pytest.mark.parametrize("t", [999, 1])
def test_residuals_low_precision(sd_lowp, t):
    sd, precision = sd_lowp
    ctx, _, lat = _inputs(BF16_DIMS)
    sd.set_control(_hints(BF16_DIMS))
    got = sd.control_residuals(lat, t, ctx)
    r64 = _residuals_ref(True, torch.float64, t)
    bar = BAR_UNET if precision == 1 else BAR_UNET_FP8
    rs = [_rel_rms(got[j], r64[j]) for j in range(13)]
    print(f"residuals precision {precision} t={t}: rel-RMS vs fp64 = " + " ".join(f"{r:.2e}" for r in rs))
    assert all(np.isfinite(g).all() for g in got) and max(rs) < bar


# ---- 4. the controlled UNet forward --------------------------------------------------------------------------------------------------------------------------
def _controlled_ref(d, dtype, t, hint, lat, ctx, strength=0.6):
    provider = syn.SyntheticWeights(cache=True)
    r = CR.ControlNetOracle(provider, d, dtype).forward(torch.from_numpy(lat), t, torch.from_numpy(ctx), CR.hint01(hint))
    return CR.controlled_forward(O.UNetOracle(provider, d, dtype), torch.from_numpy(lat), t, torch.from_numpy(ctx), r, strength).numpy()


@pytest.mark.parametrize("t", [999, 1])
def test_controlled_forward_fp32(sd, tiny_dims, t):
    d = tiny_dims
    ctx, _, lat = _inputs(d, seed=1)
    hint = _hints(d, seed=1)
    sd.set_control(hint, strength=0.6, start=0.5, end=0.5)      # (an empty window: sdmi_unet_forward ignores it, the control is on)
    got = sd.unet.forward(lat, [t], ctx)
    refs = [_controlled_ref(d, dt, t, hint, lat, ctx) for dt in (torch.float32, torch.float64)]
    e64, e32 = _assert_close(got, refs[0], refs[1], f"controlled forward t={t}")
    print(f"controlled forward t={t}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.set_control(None)
    plain = sd.unet.forward(lat, [t], ctx)
    assert np.abs(plain - got).max() > 1e-3, "the control does not reach the output"
    # one x and one context for both samples: the outputs differ through the hint alone, and swapping the hints swaps them
    # (a dark and a bright picture: eight synthetic convolutions carry little of a hint's noise, and the effect has to stand clear of the swap's own bar -- 3 x here)
    lat1, ctx1 = np.repeat(lat[:1], 2, 0), np.repeat(ctx[:1], 2, 0)
    pair = np.stack([hint[0] // 8, 255 - hint[0] // 8])
    sd.set_control(pair, strength=0.6)
    a = sd.unet.forward(lat1, [t], ctx1)
    sd.set_control(np.ascontiguousarray(pair[::-1]), strength=0.6)
    b = sd.unet.forward(lat1, [t], ctx1)
    swap_bar = 1e-5 * max(1.0, np.abs(a).max())
    print(f"controlled forward t={t}: the two hints move the outputs apart by {np.abs(a[0] - a[1]).max():.2e}; swapped to {np.abs(b - a[::-1]).max():.2e} (bar {swap_bar:.2e})")
    assert np.abs(a[0] - a[1]).max() > 3 * swap_bar, "the hint does not reach the output"
    assert np.abs(b - a[::-1]).max() <= swap_bar
    # n_hint = 1 == the same hint given twice, bit for bit
    sd.set_control(hint[:1], strength=0.6)
    one = sd.unet.forward(lat, [t], ctx)
    sd.set_control(np.repeat(hint[:1], 2, 0), strength=0.6)
    two = sd.unet.forward(lat, [t], ctx)
    assert np.array_equal(one, two)


@pytest.mark.parametrize("t", [999, 1])
def test_controlled_forward_low_precision(sd_lowp, t):
    sd, precision = sd_lowp
    d = BF16_DIMS
    ctx, _, lat = _inputs(d, seed=1)
    hint = _hints(d, seed=1)
    sd.set_control(hint, strength=0.6)
    got = sd.unet.forward(lat, [t], ctx)
    r = _rel_rms(got, _controlled_ref(d, torch.float64, t, hint, lat, ctx))
    print(f"controlled forward precision {precision} t={t}: rel-RMS vs fp64 = {r:.3e}")
    assert np.isfinite(got).all() and r < (BAR_UNET if precision == 1 else BAR_UNET_FP8)
    sd.set_control(hint[:1], strength=0.6)
    one = sd.unet.forward(lat, [t], ctx)
    sd.set_control(np.repeat(hint[:1], 2, 0), strength=0.6)
    assert np.array_equal(one, sd.unet.forward(lat, [t], ctx))


# ---- 5. identity cases: bit for bit against the same context with the control cleared --------------------------------------------------------------------------
class _ZeroedZeroConvs:
    """the context's zero convolutions and middle_block_out set to zeros for the block, the synthetic ones put back on exit"""

    def __init__(self, sd, provider):
        self.sd, self.provider = sd, provider

    def _set(self, zero):
        specs = [(n, s) for n, s in self.sd.weight_specs() if n.rsplit("/", 1)[0] in ZERO_NAMES]
        shapes = dict(self.sd.weight_specs())
        assert len(specs) == 26
        for name, shape in specs:
            self.sd.set_weight(name, np.zeros(shape, np.float32) if zero else syn.named_tensor(self.provider, name, shape, shapes))

    def __enter__(self):
        self._set(True)

    def __exit__(self, *a):
        self._set(False)


def _identity(sd, d, synth, tmp_path=None):
    ctx, unc, lat = _inputs(d, seed=2)
    hint = _hints(d, seed=2)
    sd.set_control(None)
    plain = sd.unet.forward(lat, [500], ctx)
    k_plain = sd.last_call_stats()["kernels"]
    plain_s = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
    # strength 0: the plain call, launch for launch
    sd.set_control(hint, strength=0.0)
    assert np.array_equal(sd.unet.forward(lat, [500], ctx), plain) and sd.last_call_stats()["kernels"] == k_plain
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat), plain_s)
    # all residuals zero at strength 1: the add kernel rewrites every storage form of the 13 targets with the bits their producers wrote
    lines = []
    with _ZeroedZeroConvs(sd, synth):
        assert sd.control_ready
        sd.set_control(hint, strength=1.0)
        r = sd.control_residuals(lat, 500, ctx)
        assert all(float(np.abs(v).max()) == 0.0 for v in r)
        if tmp_path is not None:
            sd.set_option("record_shapes", 1)
        try:
            got = sd.unet.forward(lat, [500], ctx)
            k = sd.last_call_stats()["kernels"]
            if tmp_path is not None:
                sd.set_option("dump_choices", str(tmp_path / "choices.txt"))
                lines = (tmp_path / "choices.txt").read_text().splitlines()
        finally:
            sd.set_option("record_shapes", 0)
        assert k > k_plain
        assert np.array_equal(got, plain), f"zero residuals at strength 1 change {int((got != plain).sum())} of {got.size} outputs"
        assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat), plain_s)
    sd.set_control(None)
    assert np.array_equal(sd.unet.forward(lat, [500], ctx), plain) and sd.last_call_stats()["kernels"] == k_plain
    return lines


def test_identity_fp32_with_plane_skips(sd, synth, tiny_dims, tmp_path):
    """model_channels = 160: every cats buffer of the fp32 engine exists as fp32 AND as bf16 planes (plane_gemm holds and 160 % 32 == 0 for both halves of each),
    so the add kernel rewrites planes at all 13 targets, and the output blocks' GEMMs read them: the recorded tile choices show plane tiles (cfg 300 ..)"""
    assert tiny_dims.model_channels % 32 == 0
    lines = _identity(sd, tiny_dims, synth, tmp_path)
    # the add launch itself: all 13 destinations carried planes next to their fp32 form
    assert "control_add segs=13 planes=13 dt=0 x1" in lines, [ln for ln in lines if "control_add" in ln]
    plane = [ln for ln in lines if re.search(r"cfg=30\d", ln)]
    print(f"{len(plane)} of {len(lines)} recorded GEMM shapes ran on plane tiles, e.g. {plane[:3]}")
    assert plane, "no GEMM of the controlled forward read planes: the plane path did not run"


def test_identity_low_precision(sd_lowp, synth):
    sd, precision = sd_lowp
    _identity(sd, BF16_DIMS, synth)


# ---- 6. sampling -------------------------------------------------------------------------------------------------------------------------------------------
def test_sample_latent_window(sd, synth, tiny_dims):
    """4 steps, start 0.25, end 0.75: steps 1 and 2 are controlled"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=3)
    hint = _hints(d, seed=3)
    sd.set_control(hint, strength=0.6, start=0.25, end=0.75)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    a = syn.alphas_cumprod()
    ts, step = O.ddim_timesteps(4)
    refs = []
    for dt in (torch.float32, torch.float64):
        pred = CR.ControlledPredictor(synth, d, dt, CR.hint01(hint), 0.6, 0.25, 0.75, len(ts))
        assert sorted(pred.on) == [1, 2]
        refs.append(CR.sample(pred, a, ctx, unc, 7.5, ts, step, lat).numpy())
    e64, e32 = _assert_close(got, refs[0], refs[1], "controlled sample_latent")
    print(f"controlled sample_latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.set_control(None)
    assert np.abs(sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat) - got).max() > 1e-3
    # cfg_share = 0 computes both halves of the UNet's shared prefix: the same latent to rounding (the control encoder computes both halves either way)
    sd.set_control(hint, strength=0.6, start=0.25, end=0.75)
    try:
        sd.set_option("cfg_share", 0)
        both = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    finally:
        sd.set_option("cfg_share", 1)
    _assert_close(both, refs[0], refs[1], "controlled sample_latent cfg_share=0")


def test_img2img_window_counts_the_tail(sd, synth, tiny_dims):
    """strength 0.5 of 4 steps runs 2: start 0, end 0.5 controls the first of THOSE (t = 499), not step 0 of the full schedule"""
    d = tiny_dims
    ctx, unc, noise = _inputs(d, seed=4)
    z0 = (np.random.default_rng(4).standard_normal((N, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    hint = _hints(d, seed=4)
    sd.set_control(hint, strength=0.6, start=0.0, end=0.5)
    got = sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=noise)
    a = syn.alphas_cumprod()
    ts, step = R.timesteps(4, 0.5)
    assert len(ts) == 2
    a0 = float(a[ts[0]])
    refs = []
    for dt in (torch.float32, torch.float64):
        pred = CR.ControlledPredictor(synth, d, dt, CR.hint01(hint), 0.6, 0.0, 0.5, len(ts))
        assert sorted(pred.on) == [0]
        x = np.sqrt(a0) * torch.from_numpy(z0).to(dt) + np.sqrt(1.0 - a0) * torch.from_numpy(noise).to(dt)
        refs.append(CR.sample(pred, a, ctx, unc, 7.5, ts, step, x).numpy())
    e64, e32 = _assert_close(got, refs[0], refs[1], "controlled img2img")
    print(f"controlled img2img: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


def test_sample_dpmpp_2m(sd, synth, tiny_dims):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=5)
    hint = _hints(d, seed=5)
    sd.set_control(hint[:1], strength=0.6)
    sd.set_sampler("dpmpp_2m")
    got = sd.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    a = syn.alphas_cumprod()
    ts, step = O.ddim_timesteps(3)
    refs = []
    for dt in (torch.float32, torch.float64):
        pred = CR.ControlledPredictor(synth, d, dt, CR.hint01(hint[:1]), 0.6, 0.0, 1.0, len(ts))
        c, u = torch.from_numpy(ctx).to(dt), torch.from_numpy(unc).to(dt)
        idx = {t: i for i, t in enumerate(ts)}
        with torch.no_grad():
            refs.append(SR.sample_textbook("dpmpp_2m", 0.0, a, ts, step, torch.from_numpy(lat).to(dt),
                                           lambda x_, t, cur: pred.forward_diffuser(x_, t, c, u, 7.5, idx[t])).numpy())
    _assert_close(got, refs[0], refs[1], "controlled sample_latent dpmpp_2m")


def test_sample_low_precision(synth):
    d = BF16_DIMS
    sd = _make(d, 1)
    try:
        sd.load_weights(synth, clip=False)
        ctx, unc, lat = _inputs(d, seed=6)
        hint = _hints(d, seed=6)
        sd.set_control(hint, strength=0.6, start=0.25, end=0.75)
        got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
        ts, step = O.ddim_timesteps(4)
        pred = CR.ControlledPredictor(syn.SyntheticWeights(cache=True), d, torch.float64, CR.hint01(hint), 0.6, 0.25, 0.75, len(ts))
        ref = CR.sample(pred, syn.alphas_cumprod(), ctx, unc, 7.5, ts, step, lat).numpy()
        r = _rel_rms(got, ref)
        print(f"controlled sample_latent precision 1: rel-RMS vs fp64 = {r:.3e}")
        assert np.isfinite(got).all() and r < BAR_LATENT
    finally:
        sd.close()


def test_dev_forms_equal_host_forms(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=7)
    z0 = (np.random.default_rng(7).standard_normal((N, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    sd.set_control(_hints(d, seed=7), strength=0.6, start=0.0, end=0.75)
    host = sd.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    host_i = sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=lat)
    dev = torch.device("cuda")
    tc, tu, tl, tz = (torch.from_numpy(v).to(dev) for v in (ctx, unc, lat, z0))
    out = torch.empty((N, 4, d.latent_h, d.latent_w), device=dev)
    torch.cuda.synchronize()
    sd.sample_latent_dev(tc.data_ptr(), N, T, tu.data_ptr(), unc.shape[0], 7.5, 3, tl.data_ptr(), out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    sd.sample_latent_from_dev(tc.data_ptr(), N, T, tu.data_ptr(), unc.shape[0], 7.5, 4, 0.5, tz.data_ptr(), None, tl.data_ptr(), 0, out.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host_i)


# ---- 7. loaders --------------------------------------------------------------------------------------------------------------------------------------------
def _f16_tensors(sd, provider):
    specs = [(n, s) for n, s in sd.weight_specs() if n.startswith("controlnet/")]
    shapes = dict(sd.weight_specs())
    return {n: syn.named_tensor(provider, n, s, shapes).astype(np.float16).astype(np.float32) for n, s in specs}


def test_loaders(synth, tiny_dims, tmp_path):
    d = tiny_dims
    ctx, _, lat = _inputs(d, seed=8)
    hint = _hints(d, seed=8)
    other = syn.SyntheticWeights(seed=11)
    sd = _make(d)
    ref = _make(d)
    try:
        # the engine's ControlNet entries are weights.control_specs' (what the writer writes)
        assert [(n, tuple(s)) for n, s in sd.weight_specs() if n.startswith("controlnet/")] == [(n, tuple(s)) for n, s in W.control_specs(d)]
        assert len(sd.weight_specs()) - len(W.control_specs(d)) == len(_make_specs_without_control(d))
        # the base model first; the ControlNet arrives BEHIND finalize_weights, from an F16 file
        sd.load_weights(synth, clip=False, control=False)
        ref.load_weights(synth, clip=False, control=False)
        assert not sd.control_ready
        assert _status(lambda: sd.set_control(hint))[0] == SDMI_ERR_STATE
        W.write_control_safetensors(tmp_path / "a.safetensors", synth, d, "F16")
        sd.load_control_safetensors(tmp_path / "a.safetensors")
        assert sd.control_ready
        for n, a in _f16_tensors(ref, synth).items():      # tensor by tensor, the fp16-rounded values
            ref.set_weight(n, a)
        assert ref.control_ready
        base = sd.unet.forward(lat, [500], ctx)
        sd.set_control(hint)
        ref.set_control(hint)
        want = ref.control_residuals(lat, 500, ctx)
        got = sd.control_residuals(lat, 500, ctx)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        # a second file replaces the first; the base model is not reloaded
        W.write_control_safetensors(tmp_path / "b.safetensors", other, d, "F32")
        sd.load_control_safetensors(tmp_path / "b.safetensors")
        got_b = sd.control_residuals(lat, 500, ctx)
        assert not np.array_equal(got_b[0], got[0])
        r64 = CR.ControlNetOracle(other, d, torch.float64).forward(torch.from_numpy(lat), 500, torch.from_numpy(ctx), CR.hint01(hint))
        r32 = CR.ControlNetOracle(other, d, torch.float32).forward(torch.from_numpy(lat), 500, torch.from_numpy(ctx), CR.hint01(hint))
        for j in range(13):
            _assert_close(got_b[j], r32[j].numpy(), r64[j].numpy(), f"second ControlNet, residual {j}")
        # three bad files: each its status, and the loaded model's residuals unchanged
        specs = W.control_specs(d)
        shapes = dict(specs)
        full = {n: syn.named_tensor(synth, n, s, shapes) for n, s in specs}
        from stable_diffusion_burn_amd import checkpoint_key
        keyed = {}
        for n, a in full.items():
            key, tr = checkpoint_key(n)
            keyed[key] = np.ascontiguousarray(a.T) if tr else a
        missing = dict(keyed)
        del missing["control_model.input_hint_block.6.bias"]
        wrong = dict(keyed)
        wrong["control_model.zero_convs.3.0.weight"] = np.zeros((d.model_channels, d.model_channels, 3, 3), np.float32)
        i64 = dict(keyed)
        i64["control_model.middle_block.1.norm.weight"] = np.zeros(4 * d.model_channels, np.int64)
        for name, tensors, status in (("missing", missing, SDMI_ERR_WEIGHTS), ("shape", wrong, SDMI_ERR_WEIGHTS), ("i64", i64, SDMI_ERR_UNSUPPORTED)):
            W.write_safetensors(tmp_path / f"{name}.safetensors", tensors)
            st, msg = _status(lambda: sd.load_control_safetensors(tmp_path / f"{name}.safetensors"))
            assert st == status, (name, st, msg)
            again = sd.control_residuals(lat, 500, ctx)
            assert all(np.array_equal(a, b) for a, b in zip(again, got_b)), name
        # a base checkpoint is no ControlNet, and the other way round
        st, _ = _status(lambda: sd.load_weights_safetensors(tmp_path / "b.safetensors"))
        assert st == SDMI_ERR_WEIGHTS
        sd.set_control(None)
        assert np.array_equal(sd.unet.forward(lat, [500], ctx), base)
        # the dump-directory route: a tree with a controlnet/ subtree
        dump = tmp_path / "dump"
        all_shapes = dict(sd.weight_specs())
        W.write_dump_tree(dump, sd.weight_specs(), lambda n, s: syn.named_tensor(other if n.startswith("controlnet/") else synth, n, s, all_shapes),
                          syn.alphas_cumprod(), n_head=d.n_head)
        assert (dump / "controlnet" / "hint" / "c2" / "stride.npy").exists()
        third = _make(d)
        try:
            third.load_weights_dir(dump)
            assert third.control_ready
            third.set_control(hint)
            got_d = third.control_residuals(lat, 500, ctx)
            assert all(np.array_equal(a, b) for a, b in zip(got_d, got_b))
        finally:
            third.close()
    finally:
        sd.close()
        ref.close()


def _make_specs_without_control(d):
    sd = _make(d, control=0)
    try:
        return sd.weight_specs()
    finally:
        sd.close()


# ---- 8. statuses -------------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(sd, sd_tiny, tiny_dims, synth):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=9)
    hint = _hints(d, seed=9)
    # sdmi_create
    for bad, status in ((1, SDMI_ERR_INVALID), (4, SDMI_ERR_INVALID), (-3, SDMI_ERR_INVALID)):
        assert _status(lambda: _make(d, control=bad))[0] == status
    assert _status(lambda: StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, 16, 16, d.vae_ch, unet_in_ch=9, control_hint_ch=3)))[0] == SDMI_ERR_UNSUPPORTED
    # a context without a ControlNet
    assert _status(lambda: sd_tiny.set_control(hint))[0] == SDMI_ERR_STATE
    assert _status(lambda: sd_tiny.load_control_safetensors("/nonexistent.safetensors"))[0] == SDMI_ERR_STATE
    assert _status(lambda: sd_tiny.control_hint_embed(hint))[0] == SDMI_ERR_STATE
    assert not sd_tiny.control_ready
    sd_tiny.unet.forward(lat, [500], ctx)
    # sdmi_set_control: refused, and the state unchanged
    sd.set_control(hint, strength=0.6)
    want = sd.unet.forward(lat, [500], ctx)
    for kw in (dict(strength=float("nan")), dict(strength=float("inf")), dict(start=0.6, end=0.5), dict(start=-0.1), dict(end=1.5), dict(start=float("nan"))):
        st, msg = _status(lambda: sd.set_control(hint, **kw))
        assert st == SDMI_ERR_INVALID, (kw, st, msg)
        assert np.array_equal(sd.unet.forward(lat, [500], ctx), want), kw
    from stable_diffusion_burn_amd._capi import SdmiControl
    c = SdmiControl()
    c.n_hint, c.hint_h, c.hint_w, c.strength, c.start, c.end = 1, 128, 128, 1.0, 0.0, 1.0
    assert sd._lib.sdmi_set_control(sd._ctx, C.byref(c)) == SDMI_ERR_INVALID        # a null hint
    c.hint_rgb = hint.ctypes.data_as(C.POINTER(C.c_uint8))
    c.n_hint = 0
    assert sd._lib.sdmi_set_control(sd._ctx, C.byref(c)) == SDMI_ERR_INVALID
    assert np.array_equal(sd.unet.forward(lat, [500], ctx), want)
    # a forward whose latent size is not hint / 8, a call with another n: both sizes named
    sd.set_latent_size(8, 24)
    st, msg = _status(lambda: sd.unet.forward(np.zeros((2, 4, 8, 24), np.float32), [500], ctx))
    assert st == SDMI_ERR_INVALID and "128 x 128" in msg and "8 x 24" in msg, msg
    sd.set_control(_hints(d, h=8, w=24, seed=9), strength=0.6)        # set_latent_size followed by a matching set_control works, non-square
    assert np.isfinite(sd.unet.forward(lat[:, :, :8, :8].repeat(3, axis=3), [500], ctx)).all()
    sd.set_latent_size(d.latent_h, d.latent_w)
    sd.set_control(hint, strength=0.6)
    st, msg = _status(lambda: sd.unet.forward(lat[:1], [500], ctx[:1]))
    assert st == SDMI_ERR_INVALID and "n = 1" in msg and "n_hint = 2" in msg, msg
    st, msg = _status(lambda: sd.sample_latent(np.repeat(ctx, 2, 0)[:3], unc, 7.5, 2, init_latent=np.repeat(lat, 2, 0)[:3]))
    assert st == SDMI_ERR_INVALID and "n = 3" in msg, msg
    assert np.array_equal(sd.unet.forward(lat, [500], ctx), want)
    # hires while a control is set
    st, msg = _status(lambda: sd.sample_latent_hires(ctx, unc, 7.5, 2, (8, 8), 0.5, init_latent=lat[:, :, :8, :8]))
    assert st == SDMI_ERR_UNSUPPORTED, (st, msg)
    assert np.array_equal(sd.unet.forward(lat, [500], ctx), want)
    sd.set_control(None)
    assert np.isfinite(sd.sample_latent_hires(ctx, unc, 7.5, 2, (8, 8), 0.5, init_latent=np.ascontiguousarray(lat[:, :, :8, :8]))).all()
    # control_residuals without a control
    assert _status(lambda: sd.control_residuals(lat, 500, ctx))[0] == SDMI_ERR_STATE
    # a partial group is refused by finalize_weights
    part = _make(d)
    try:
        part.load_weights(synth, clip=False, control=False)
        shapes = dict(part.weight_specs())
        for name, shape in W.control_specs(d):
            if name != "controlnet/zero_convs/5/bias":
                part.set_weight(name, syn.named_tensor(synth, name, shape, shapes))
        assert not part.control_ready
        assert part._lib.sdmi_finalize_weights(part._ctx) == SDMI_ERR_WEIGHTS
        msg = part._lib.sdmi_last_error().decode()
        assert "ControlNet" in msg and "controlnet/zero_convs/5/bias" in msg, msg
        part.set_weight("controlnet/zero_convs/5/bias", syn.named_tensor(synth, "controlnet/zero_convs/5/bias", shapes["controlnet/zero_convs/5/bias"], shapes))
        assert part._lib.sdmi_finalize_weights(part._ctx) == 0 and part.control_ready
    finally:
        part.close()


def test_sharded_refuses_a_set_control(synth, tiny_dims):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    d = tiny_dims
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, control_hint_ch=3), devices=(0,))
    try:
        m.load_weights(synth)
        ctx, unc, lat = _inputs(d, seed=10)
        m.device_view(0).set_control(_hints(d, seed=10))
        st, msg = _status(lambda: m.sample_image(ctx[0], unc, 7.5, 1, 2, init_latents=lat))
        assert st == SDMI_ERR_UNSUPPORTED, (st, msg)
        m.device_view(0).set_control(None)
        assert m.sample_image(ctx[0], unc, 7.5, 1, 2, init_latents=lat).shape == (2, 8 * d.latent_h, 8 * d.latent_w, 3)
    finally:
        m.close()


# ---- 9. scratch independence -----------------------------------------------------------------------------------------------------------------------------------
def test_scratch_fill(sd, tiny_dims, tmp_path):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=11)
    sd.set_control(_hints(d, seed=11), strength=0.6)
    _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), "controlled unet.forward")
    _sweep(sd, tmp_path, lambda: sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat), "controlled 2-step sample_latent")
    _sweep(sd, tmp_path, lambda: sd.control_hint_embed(_hints(d, seed=11)), "control_hint_embed")


def test_scratch_fill_low_precision(sd_lowp, tmp_path):
    sd, precision = sd_lowp
    d = BF16_DIMS
    ctx, unc, lat = _inputs(d, seed=11)
    sd.set_control(_hints(d, seed=11), strength=0.6)
    _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), f"controlled unet.forward precision {precision}")
    _sweep(sd, tmp_path, lambda: sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat), f"controlled 2-step sample_latent precision {precision}")


# ---- 10. no cost when off ------------------------------------------------------------------------------------------------------------------------------------
# Launch counts of this module's tiny model (n = 2, T = 7, fp32).  PARENT_*: the commit before this feature, measured by running its library on the same two calls.
PARENT_FORWARD_LAUNCHES = 587
PARENT_SAMPLE2_LAUNCHES = 1097
# What DESIGN.md section 9g lists.  To prepare a controlled call: per hint picture 1 conversion + 8 convolutions + 7 SiLU (2 x 16), the ControlNet's time MLP (2 GEMMs + 2 SiLU),
# one row GEMM per control ResBlock (6 + 2 + the middle block's 2 = 10) and K / V per control transformer (2 x 7): 60 launches, and the 17 split-K reduce launches the
# planner adds to them at these shapes.
CONTROL_PREPARE_LAUNCHES = 77
# Per controlled step: the control encoder and middle block on the whole batch, 13 zero convolutions (split-K reduces included) and ONE add.
CONTROL_STEP_LAUNCHES = 251


def test_no_cost_when_off(sd, sd_tiny, tiny_dims):
    """A context without a ControlNet, one with a ControlNet and the control cleared, and the commit before the feature all launch the same kernels for the same
    forward and give the same bits; a controlled forward adds exactly what DESIGN.md section 9g lists."""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=12)
    plain = sd_tiny.unet.forward(lat, [500], ctx)
    k0 = sd_tiny.last_call_stats()["kernels"]
    sd.set_control(None)
    cleared = sd.unet.forward(lat, [500], ctx)
    k1 = sd.last_call_stats()["kernels"]
    assert np.array_equal(plain, cleared) and k0 == k1
    assert k0 == PARENT_FORWARD_LAUNCHES
    s0 = sd_tiny.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
    ks0 = sd_tiny.last_call_stats()["kernels"]
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat), s0) and sd.last_call_stats()["kernels"] == ks0 == PARENT_SAMPLE2_LAUNCHES
    assert len(sd_tiny.weight_specs()) + 340 == len(sd.weight_specs())
    # What a controlled call adds, by the step window of a 2-step sample: with an EMPTY window the call only prepares -- the hint (per picture 1 conversion +
    # 8 convolutions + 7 SiLU), the control time MLP (2 GEMMs + 2 SiLU), one row GEMM per control ResBlock (10) and K / V per control transformer (2 x 7), their split-K reduces --, and every
    # controlled step adds the same launches: the control encoder (the UNet's own encoder and middle block, both CFG halves), 13 zero convolutions and ONE add.
    hint = _hints(d, seed=12)

    def launches(start, end):
        sd.set_control(hint, strength=0.6, start=start, end=end)
        sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
        return sd.last_call_stats()["kernels"]

    k_empty, k_first, k_second, k_both = launches(0.5, 0.5), launches(0.0, 0.5), launches(0.5, 1.0), launches(0.0, 1.0)
    prepare, per_step = k_empty - ks0, k_first - k_empty
    sd.set_control(hint, strength=0.6)
    sd.unet.forward(lat, [500], ctx)
    k2 = sd.last_call_stats()["kernels"]
    print(f"launches: plain forward {k0}, controlled forward {k2} (+{k2 - k0}); 2-step sample {ks0}, + {prepare} to prepare a controlled call, + {per_step} per controlled step")
    assert k_second - k_empty == per_step and k_both - k_empty == 2 * per_step
    assert prepare == CONTROL_PREPARE_LAUNCHES and per_step == CONTROL_STEP_LAUNCHES
    assert k2 - k0 == CONTROL_PREPARE_LAUNCHES + CONTROL_STEP_LAUNCHES      # a forward is a one-step call, its control always on
