"""FreeU on the GPU (include/sdmi.h "FreeU"), through the C ABI, against the CPU restatement in tests/freeu_ref.py.  Every bar is a
neighbouring module's: test_views_gpu (operator level), test_img2img_gpu (fp32 model level: the GPU's error against the fp64 oracle held against the fp32 oracle's own),
test_bf16_gpu / test_controlnet_gpu (relative RMS at precisions 1 / 2), test_scratch_fill_gpu (the pool_fill sweep).

Measured on an MI355X (the figures the tests print; DESIGN.md section 9l repeats them): operator level 1.1e-7 (precision 0) and 3.1e-3 (precisions 1 / 2) of
max(1, max|ref|); fp32 forwards |gpu - f64| 1.4 .. 1.6e-6 (the f32 oracle's own: 1.3 .. 1.5e-6), 4-step samples 1.3e-4 (1.2 .. 1.3e-4); rel-RMS of a forward at
precision 1: 1.05e-2 (v1) / 1.08e-2 (v2) against 1.01e-2 with FreeU off, at precision 2: 8.57e-2 / 8.62e-2 against 8.34e-2."""
import functools

import numpy as np
import pytest
import torch

import controlnet_ref as CR
import freeu_ref as FR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn
from test_bf16_gpu import BAR_UNET
from test_hires_gpu import BF16_DIMS
from test_img2img_gpu import _assert_close
from test_scratch_fill_gpu import _sweep
from test_views_gpu import BF16_BAR, FP32_BAR, _check, bf16_round

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED = -1, -5
BAR_UNET_FP8 = 1.28e-1     # tests/test_controlnet_gpu.py / test_fp8_gpu.py: rel-RMS of a UNet forward at precision 2 against the exact fp64 oracle
N, T = 2, 7
PARAMS = dict(b1=1.3, b2=1.4, s1=0.9, s2=0.2)
PAIRS = [(1.3, 0.9), (1.6, 0.2), (1.0, 0.5), (1.4, 1.0)]
# (cx, cskip, H, W): one granule each at the smallest sizes (1 x 3: F(H) = {0}; 2 x 2: every mode real), a pixel count that is no multiple of any lane count, and the
# headline model's widths at a size of several passes per thread
SHAPES = [(64, 32, 1, 3), (64, 64, 2, 2), (128, 96, 5, 7), (640, 320, 24, 40)]
LONGEST = (640, 320, 64, 64)      # the longest pixel walk of the headline model: 4096 pixels per workgroup


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _status(fn):
    from stable_diffusion_burn_amd import SdmiError
    try:
        fn()
    except SdmiError as e:
        return e.status, str(e)
    return 0, ""


def _make(d, precision=0, **kw):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    return StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision, **kw))


# ---- 1. operator level --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1, 2])
def ops(request):
    sd = _make(O.Dims(64, 1, 64, 8, 8, 64), request.param)
    yield sd, request.param
    sd.close()


def _shape_for(shape, precision):
    """at precisions 1 and 2 a slice is 64 channels wide: the 32-wide cases become 64"""
    cx, cskip, h, w = shape
    if precision:
        cx, cskip = max(cx, 128), (cskip + 63) // 64 * 64
    return cx, cskip, h, w


def _op_input(shape, precision, seed):
    cx, cskip, h, w = shape
    g = np.random.default_rng(seed)
    x = g.standard_normal((N, cx + cskip, h, w)).astype(np.float32)
    x[1] = x[1] * 1.7 + 0.3                      # the two samples of a call differ in more than their noise
    x[:, cx:] += g.standard_normal((N, cskip, 1, 1)).astype(np.float32)     # a mean per skip channel: the zero frequency carries weight
    return bf16_round(x) if precision else x     # the storage type's own rounding of the input is not the operator's error


def _op_case(sd, precision, shape, version, b, s, seed=0):
    cx, cskip, h, w = shape
    x = _op_input(shape, precision, seed)
    y, yp = sd.op_freeu(x, cx, version, b, s, planes=True)
    what = f"op_freeu precision {precision} {shape} v{version} b={b} s={s}"
    ref = FR.op(x, cx, version, b, s)
    err = np.abs(y - ref).max() / max(1.0, np.abs(ref).max())
    print(f"{what}: max|d| / max(1, |ref|) = {err:.3e}")
    _check(y, ref, what, BF16_BAR if precision else FP32_BAR)
    if precision == 0:
        assert yp is not None, f"{what}: the buffer had no planes"
        assert np.array_equal(_bits(yp), _bits(y)), f"{what}: the planes hold other bits than the fp32 copy"
    else:
        assert yp is None
    # untouched halves keep their bits
    if b == 1.0:
        assert np.array_equal(_bits(y[:, :cx]), _bits(x[:, :cx])), what
    else:
        assert np.array_equal(_bits(y[:, cx // 2:cx]), _bits(x[:, cx // 2:cx])), what
    if s == 1.0:
        assert np.array_equal(_bits(y[:, cx:]), _bits(x[:, cx:])), what
    return x, y


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_op_freeu(ops, shape, version):
    sd, precision = ops
    shape = _shape_for(shape, precision)
    for i, (b, s) in enumerate(PAIRS):
        x, y = _op_case(sd, precision, shape, version, b, s, seed=10 * version + i)
        if i == 0:
            # determinism, and each sample's result does not depend on the batch it is in
            again = sd.op_freeu(x, shape[0], version, b, s)
            assert np.array_equal(_bits(again), _bits(y))
            for k in range(N):
                one = sd.op_freeu(x[k:k + 1], shape[0], version, b, s)
                assert np.array_equal(_bits(one[0]), _bits(y[k])), f"sample {k} alone gives other bits than in the batch"


def test_op_freeu_longest_pixel_walk(ops):
    sd, precision = ops
    _op_case(sd, precision, _shape_for(LONGEST, precision), 2, 1.3, 0.9, seed=99)


@pytest.mark.parametrize("shape", [(64, 32, 1, 1), (64, 32, 1, 3), (128, 96, 5, 7)])
def test_op_freeu_v2_constant_mean(ops, shape):
    """max m == min m: the published code divides by zero; here m_hat = 0 and the backbone keeps its bits.  Channel 2k + 1 = -channel 2k makes every pixel's channel
    sum exactly zero in any order of pairwise-adjacent adds (a 1 x 1 level is constant by itself)."""
    sd, precision = ops
    cx, cskip, h, w = _shape_for(shape, precision)
    x = _op_input((cx, cskip, h, w), precision, 7)
    if h * w > 1:
        x[:, 1:cx:2] = -x[:, 0:cx:2]
    y = sd.op_freeu(x, cx, 2, 1.6, 0.5)
    assert np.array_equal(_bits(y[:, :cx]), _bits(x[:, :cx])), "m_hat must be 0 where max == min"
    _check(y, FR.op(x, cx, 2, 1.6, 0.5), f"constant-mean {shape} precision {precision}", BF16_BAR if precision else FP32_BAR)


def test_op_freeu_refusals(ops):
    sd, precision = ops
    x = np.zeros((1, 256, 2, 2), np.float32)
    assert _status(lambda: sd.op_freeu(x, 128, 3, 1.2, 0.9))[0] == SDMI_ERR_INVALID
    assert _status(lambda: sd.op_freeu(x, 128, 1, 0.0, 0.9))[0] == SDMI_ERR_INVALID
    assert _status(lambda: sd.op_freeu(x, 128, 1, 1.2, -0.5))[0] == SDMI_ERR_INVALID
    assert _status(lambda: sd.op_freeu(x, 256, 1, 1.2, 0.9))[0] == SDMI_ERR_INVALID
    assert _status(lambda: sd.op_freeu(x, 48, 1, 1.2, 0.9))[0] == SDMI_ERR_UNSUPPORTED        # cx / 2 = 24
    assert _status(lambda: sd.op_freeu(x, 128 + 16, 1, 1.2, 0.9))[0] == SDMI_ERR_UNSUPPORTED


# ---- 2. model level, fp32 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sdc(tiny_dims, synth):
    """the module's fp32 context: the tiny model with a ControlNet beside it (cleared, it runs the plain model's launches)"""
    sd = _make(tiny_dims, control_hint_ch=3)
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture
def sd(sdc, tiny_dims):
    yield sdc
    sdc.set_freeu(None)
    sdc.set_control(None)
    sdc.set_sampler(None)
    sdc.set_latent_size(tiny_dims.latent_h, tiny_dims.latent_w)


def _inputs(d, n=N, seed=0, h=None, w=None):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(3, d.ctx_dim)
    lat = np.stack([syn.initial_latent(70 + seed + i, h or d.latent_h, w or d.latent_w) for i in range(n)])
    return ctx, unc, lat


@functools.lru_cache(maxsize=None)
def _forward_ref(wide: bool, dtype, version, size, t=500):
    d = BF16_DIMS if wide else O.Dims(160, 4, 64, 16, 16, 32)
    ctx, _, lat = _inputs(d, seed=1, h=size[0], w=size[1])
    unet = O.UNetOracle(syn.SyntheticWeights(cache=True), d, dtype)
    p = FR.Params(version=version, **PARAMS) if version else None
    return FR.freeu_forward(unet, torch.from_numpy(lat), t, torch.from_numpy(ctx), p).numpy()


def _choices(sd, tmp_path, fn):
    path = tmp_path / "choices.txt"
    try:
        sd.set_option("record_shapes", 1)
        out = fn()
        sd.set_option("dump_choices", str(path))
    finally:
        sd.set_option("record_shapes", 0)
    return out, path.read_text().splitlines()


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("size", [(16, 16), (8, 24)])
def test_forward_fp32(sd, tiny_dims, tmp_path, size, version):
    """unet.forward with FreeU against freeu_forward (the published FFT code inside the oracle), at the configured size and after set_latent_size(8, 24), where the
    deepest level is 1 x 3.  mc = 160: every cats buffer carries planes, so the filter rewrites planes on all ten skips."""
    d = tiny_dims
    assert d == O.Dims(160, 4, 64, 16, 16, 32)
    sd.set_latent_size(*size)
    ctx, _, lat = _inputs(d, seed=1, h=size[0], w=size[1])
    sd.set_freeu(version=version, start=0.5, end=0.5, **PARAMS)       # (an empty window: sdmi_unet_forward ignores it, FreeU is on)
    assert sd.get_freeu() == {"version": version, "start": 0.5, "end": 0.5, **{k: pytest.approx(v, rel=1e-7) for k, v in PARAMS.items()}}
    got, lines = _choices(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx))
    e64, e32 = _assert_close(got, _forward_ref(False, torch.float32, version, size), _forward_ref(False, torch.float64, version, size), f"FreeU v{version} forward {size}")
    print(f"FreeU v{version} forward {size}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    assert "freeu_filter segs=10 planes=10 dt=0 x1" in lines, [ln for ln in lines if "freeu" in ln]
    bb = [ln for ln in lines if ln.startswith("freeu_backbone")]
    assert sum(int(ln.rsplit(" x", 1)[1]) for ln in bb) == 10 and all(f"v{version} " in ln and "planes=1 dt=0" in ln for ln in bb), bb
    assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(got)), "two runs give different bits"
    sd.set_freeu(None)
    assert sd.get_freeu() is None
    plain = sd.unet.forward(lat, [500], ctx)
    assert np.abs(plain - got).max() > 1e-3, "FreeU does not reach the output"
    _assert_close(plain, _forward_ref(False, torch.float32, 0, size), _forward_ref(False, torch.float64, 0, size), f"plain forward {size}")


def _sample_refs(synth, d, params, ctx, unc, lat, window, control=None):
    a = syn.alphas_cumprod()
    ts, step = O.ddim_timesteps(4)
    refs = []
    for dt in (torch.float32, torch.float64):
        c = None
        if control is not None:
            hint, strength = control
            c = (CR.ControlNetOracle(synth, d, dt), CR.hint01(hint), strength)
        pred = FR.FreeUPredictor(synth, d, dt, params, window[0], window[1], len(ts), control=c)
        assert sorted(pred.on) == [1, 2]
        refs.append(CR.sample(pred, a, ctx, unc, 7.5, ts, step, lat).numpy())
    return refs


@pytest.mark.parametrize("version", [1, 2])
def test_sample_latent_window(sd, synth, tiny_dims, version):
    """4 steps, start 0.25, end 0.75: FreeU is on in steps 1 and 2, both CFG halves alike (the shared CFG prefix stays shared)"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=3)
    sd.set_freeu(version=version, start=0.25, end=0.75, **PARAMS)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    refs = _sample_refs(synth, d, FR.Params(version=version, **PARAMS), ctx, unc, lat, (0.25, 0.75))
    e64, e32 = _assert_close(got, refs[0], refs[1], f"FreeU v{version} sample_latent")
    print(f"FreeU v{version} sample_latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.set_freeu(None)
    assert np.abs(sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat) - got).max() > 1e-3


def test_sample_latent_with_a_control(sd, synth, tiny_dims):
    """the order: the control adds to the saved skips and the middle block's output first, FreeU works on the sums"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=4)
    g = np.random.default_rng(904)
    hint = g.integers(0, 256, (N, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=np.uint8)
    hint[1] //= 4
    sd.set_control(hint, strength=0.6)
    sd.set_freeu(version=1, start=0.25, end=0.75, **PARAMS)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    refs = _sample_refs(synth, d, FR.Params(version=1, **PARAMS), ctx, unc, lat, (0.25, 0.75), control=(hint, 0.6))
    e64, e32 = _assert_close(got, refs[0], refs[1], "FreeU + ControlNet sample_latent")
    print(f"FreeU + ControlNet sample_latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


# ---- 3. model level, precisions 1 and 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 2])
def sd_lowp(request, synth):
    sd = _make(BF16_DIMS, request.param)
    sd.load_weights(synth, clip=False)
    if request.param == 2:
        sd.set_option("fp8_min_rows", 1)     # 16 x 16 latents have few rows per GEMM: the MXFP8 path anyway (tests/test_fp8_gpu.py)
    yield sd, request.param
    sd.close()


@pytest.mark.parametrize("version", [1, 2])
def test_forward_low_precision(sd_lowp, version):
    """relative RMS against the fp64 freeu_forward, held to the plain forward's bars; the plain forward's figure on the same inputs is printed beside it
    (measured: the module's docstring)."""
    sd, precision = sd_lowp
    d = BF16_DIMS
    size = (d.latent_h, d.latent_w)
    ctx, _, lat = _inputs(d, seed=1)
    bar = BAR_UNET if precision == 1 else BAR_UNET_FP8
    try:
        sd.set_freeu(None)
        plain = sd.unet.forward(lat, [500], ctx)
        r_off = _rel_rms(plain, _forward_ref(True, torch.float64, 0, size))
        sd.set_freeu(version=version, **PARAMS)
        got = sd.unet.forward(lat, [500], ctx)
        r_on = _rel_rms(got, _forward_ref(True, torch.float64, version, size))
        print(f"precision {precision} FreeU v{version}: rel-RMS vs fp64 = {r_on:.3e} (FreeU off, same inputs: {r_off:.3e}; bar {bar:.3e})")
        assert np.isfinite(got).all() and r_off < bar
        assert r_on < bar
        assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(got))
    finally:
        sd.set_freeu(None)


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(sd, sd_tiny, tiny_dims):
    """cleared, all four parameters at 1, an empty window: the bits and the launch count of a context that never heard of FreeU.  On: exactly 1 filter launch per
    forward and 1 (version 1) or 2 (version 2) launches per affected block."""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=5)
    sd_tiny.set_latent_size(d.latent_h, d.latent_w)
    want = sd_tiny.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    k_want = sd_tiny.last_call_stats()["kernels"]
    states = {"cleared": lambda: sd.set_freeu(None), "all ones": lambda: sd.set_freeu(1.0, 1.0, 1.0, 1.0, version=2),
              "empty window": lambda: sd.set_freeu(version=1, start=0.4, end=0.4, **PARAMS)}
    for name, setter in states.items():
        sd.set_freeu(version=2, **PARAMS)      # from a state that is on
        setter()
        got = sd.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
        assert np.array_equal(_bits(got), _bits(want)), name
        assert sd.last_call_stats()["kernels"] == k_want, name
    plain = sd_tiny.unet.forward(lat, [500], ctx)
    k0 = sd_tiny.last_call_stats()["kernels"]
    for version, extra in ((1, 1 + 10), (2, 1 + 20)):
        sd.set_freeu(version=version, **PARAMS)
        got = sd.unet.forward(lat, [500], ctx)
        assert sd.last_call_stats()["kernels"] - k0 == extra, version
        assert np.abs(got - plain).max() > 1e-3
    # a group at b == 1 runs no backbone launch, one at s == 1 contributes no segment
    sd.set_freeu(1.3, 1.0, 1.0, 0.2, version=1)
    sd.unet.forward(lat, [500], ctx)
    assert sd.last_call_stats()["kernels"] - k0 == 1 + 7
    sd.set_freeu(1.0, 1.0, 1.0, 0.2, version=2)
    sd.unet.forward(lat, [500], ctx)
    assert sd.last_call_stats()["kernels"] - k0 == 1
    sd.set_freeu(1.0, 1.4, 1.0, 1.0, version=2)
    sd.unet.forward(lat, [500], ctx)
    assert sd.last_call_stats()["kernels"] - k0 == 6


# ---- 5. scratch independence, refusals, the sharded call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_scratch_fill(sd, tiny_dims, tmp_path, version):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=6)
    sd.set_freeu(version=version, **PARAMS)
    _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), f"FreeU v{version} unet.forward")


@pytest.mark.parametrize("version", [1, 2])
def test_scratch_fill_low_precision(sd_lowp, tmp_path, version):
    sd, precision = sd_lowp
    ctx, unc, lat = _inputs(BF16_DIMS, seed=6)
    try:
        sd.set_freeu(version=version, **PARAMS)
        _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), f"FreeU v{version} unet.forward precision {precision}")
    finally:
        sd.set_freeu(None)


def test_refusals(sd, tiny_dims):
    d = tiny_dims
    # model_channels = 16: cx / 2 = 16 in the second group, below the kernels' granule.  sdmi_create itself takes model_channels in multiples of 32 only (64 at
    # precisions 1 and 2) -- the same granules -- so such a context is refused there, before set_freeu's own SDMI_ERR_UNSUPPORTED can be reached; were it ever
    # created, set_freeu must refuse it and keep the state.  The granule rule itself is exercised through sdmi_op_freeu (test_op_freeu_refusals).
    made = []
    st, msg = _status(lambda: made.append(_make(O.Dims(16, 1, 64, 8, 8, 32))))
    if made:
        narrow = made[0]
        try:
            st, msg = _status(lambda: narrow.set_freeu(version=1, **PARAMS))
            assert st == SDMI_ERR_UNSUPPORTED and "multiples of 32" in msg, (st, msg)
            assert narrow.get_freeu() is None
        finally:
            narrow.close()
    else:
        assert st == SDMI_ERR_INVALID and "multiple of 32" in msg, (st, msg)
    ctx, _, lat = _inputs(d, seed=7)
    sd.set_freeu(version=2, start=0.25, end=0.75, **PARAMS)
    state = sd.get_freeu()
    want = sd.unet.forward(lat, [500], ctx)
    for bad in (dict(version=3, **PARAMS), dict(version=1, **{**PARAMS, "b1": 0.0}), dict(version=1, **{**PARAMS, "b2": -1.0}), dict(version=1, **{**PARAMS, "s2": -0.1}),
                dict(version=1, start=0.6, end=0.5, **PARAMS), dict(version=1, end=1.5, **PARAMS), dict(version=1, **{**PARAMS, "s1": float("nan")})):
        st, msg = _status(lambda: sd.set_freeu(**bad))
        assert st == SDMI_ERR_INVALID and "freeu" in msg, (bad, st, msg)
        assert sd.get_freeu() == state, "a refused setting changed the state"
    assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(want)), "the earlier setting is no longer in force"


def test_sharded_call_gives_the_single_contexts_bits(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    d = tiny_dims
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=(0,))
    try:
        m.load_weights(synth)
        n = 3
        lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(n)])
        ctx, unc = syn.cond_context(0, T, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        plain = m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat)
        m.set_freeu(version=2, **PARAMS)
        sd.set_freeu(version=2, **PARAMS)
        got = m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat)
        ref = sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 2, init_latent=lat)
        assert np.array_equal(got, ref)
        assert (got != plain).any(), "FreeU does not reach the sharded call"
        st, msg = _status(lambda: m.set_freeu(version=5, **PARAMS))
        assert st == SDMI_ERR_INVALID
        m.set_freeu(None)
        assert np.array_equal(m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat), plain)
    finally:
        m.close()
