"""IP-Adapter on the GPU (include/sdmi.h "IP-Adapter"), through the C ABI, against the CPU restatement in tests/ip_adapter_ref.py.  Every bar
is a neighbouring module's: test_views_gpu (operator level, tokens, K_ip / V_ip), test_img2img_gpu (fp32 model level: the GPU's error against the fp64 oracle held
against the fp32 oracle's own), test_bf16_gpu / test_controlnet_gpu (relative RMS at precisions 1 / 2), test_scratch_fill_gpu (the pool_fill sweep).

Measured on an MI355X (the figures the tests print; DESIGN.md section 9m repeats them): operator level 2.5e-7 (precision 0) and 3.6e-3 (precisions 1 / 2) of
max(1, max|ref|); image_proj 4.1e-7, hoisted K_ip / V_ip 4.0e-7; fp32 forward |gpu - f64| 1.4e-6 (the f32 oracle's own: 1.3e-6), 4-step samples 1.1e-4 (1.1e-4),
first-half window 1.7e-4 (1.2e-4), with a ControlNet 1.5e-4 (1.3e-4), img2img 1.3e-5 (1.1e-5); rel-RMS of a forward at precision 1: 9.6e-3 against 1.01e-2 with the
adapter off, at precision 2: 7.8e-2 against 8.3e-2; of a 4-step sample_latent: 1.42e-2 against 1.50e-2, and 1.04e-1 against 1.02e-1; with a ControlNet set a forward
9.7e-3 against 9.8e-3 and 7.2e-2 against 7.7e-2, a 4-step sample_latent 1.51e-2 and 1.06e-1; sample_latent_from (the last 2 of 4 steps) 1.28e-2 and 8.8e-2 (bars 1.7e-2 /
1.28e-1).
"""
import functools

import numpy as np
import pytest
import torch

import controlnet_ref as CR
import img2img_ref as R
import ip_adapter_ref as IR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd.weights import write_ip_adapter_safetensors
from test_bf16_gpu import BAR_UNET
from test_hires_gpu import BF16_DIMS
from test_img2img_gpu import _assert_close
from test_scratch_fill_gpu import _sweep
from test_views_gpu import BF16_BAR, FP32_BAR, _check, bf16_round

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED, SDMI_ERR_STATE = -1, -5, -6
BAR_UNET_FP8 = 1.28e-1     # tests/test_controlnet_gpu.py / test_fp8_gpu.py: rel-RMS of a UNet forward at precision 2 against the exact fp64 oracle
N, T = 2, 7
D_EMB, T_IMG = 64, 4       # the synthetic adapter: a 64-wide image embedding, 4 tokens per picture
SCALE = 0.8
# (n, nq, T_ip, heads, d): rows that fill no wave, one key, key counts that are no multiple of 4 or 32, more than one 64-row workgroup, the four head widths, and
# one at the headline model's width
SHAPES = [(2, 3, 1, 4, 40), (2, 7, 4, 2, 80), (2, 33, 16, 1, 160), (2, 65, 33, 1, 64), (2, 130, 64, 4, 40), (2, 256, 4, 8, 40)]


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


def _op_input(shape, precision, seed):
    n, nq, tip, heads, d = shape
    c = heads * d
    g = np.random.default_rng(seed)
    q, o = (g.standard_normal((n, nq, c)).astype(np.float32) for _ in range(2))
    k, v = (g.standard_normal((n, tip, c)).astype(np.float32) for _ in range(2))
    for a in (q, o, k, v):
        a[1] = a[1] * 1.7 + 0.3                    # the two samples of a call differ in more than their noise
    if precision:                                  # the storage type's own rounding of q and O_text is not the operator's error; K_ip / V_ip stay fp32
        q, o = bf16_round(q), bf16_round(o)
    return q, k, v, o


def _stored_q(q, d, precision):
    """q as the context STORES it, back in natural units.  A bf16 context keeps the queries of the head widths its fused bf16 attention serves (40, 80, 160 on an SD v1
    context) multiplied by d^-1/2 log2(e) -- folded into the query weights at load, applied by the operator entry's conversion -- so the stored tensor is
    bf16(q c), not bf16(q): that rounding is the storage type's, like the one of O_text, and the reference starts from the stored value."""
    if not precision or d not in (40, 80, 160):
        return np.asarray(q, np.float64)
    c = np.float32(1.4426950408889634 / np.sqrt(float(d)))
    return bf16_round(np.asarray(q, np.float32) * c).astype(np.float64) / np.float64(c)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_ip_attention(ops, shape):
    sd, precision = ops
    n, nq, tip, heads, d = shape
    q, k, v, o = _op_input(shape, precision, sum(shape))
    bar = BF16_BAR if precision else FP32_BAR
    for scale in ([0.7, 0.0], [0.5, 1.25]):
        s = np.asarray(scale, np.float32)
        what = f"op_ip_attention precision {precision} {shape} scale {scale}"
        got = sd.op_ip_attention(q, k, v, o, s, heads)
        ref = IR.op(_stored_q(q, d, precision), k, v, o, s, heads)
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        print(f"{what}: max|d| / max(1, |ref|) = {err:.3e} (bar {bar:.3e})")
        _check(got, ref, what, bar)
        for b in range(n):
            if scale[b] == 0.0:
                assert np.array_equal(_bits(got[b]), _bits(o[b])), f"{what}: the row with scale 0 lost O_text's bits"
            else:
                assert np.abs(got[b] - o[b]).max() > 1e-2, f"{what}: sample {b} did not move"
        # two runs, and each sample alone: the same bits
        assert np.array_equal(_bits(sd.op_ip_attention(q, k, v, o, s, heads)), _bits(got)), f"{what}: two runs differ"
        for b in range(n):
            one = sd.op_ip_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], o[b:b + 1], s[b:b + 1], heads)
            assert np.array_equal(_bits(one[0]), _bits(got[b])), f"{what}: sample {b} alone gives other bits than in the batch"
        if precision == 0:     # the plane form: read-modify-write of the three bf16 planes holds the bits of the fp32 result
            planes = sd.op_ip_attention(q, k, v, o, s, heads, planes=True)
            assert np.array_equal(_bits(planes), _bits(got)), f"{what}: the planes hold other bits than the fp32 result"


def test_op_refusals(ops):
    sd, precision = ops
    z = lambda *s: np.zeros(s, np.float32)     # noqa: E731
    one = np.ones(1, np.float32)
    assert _status(lambda: sd.op_ip_attention(z(1, 4, 160), z(1, 65, 160), z(1, 65, 160), z(1, 4, 160), one, 4))[0] == SDMI_ERR_UNSUPPORTED     # T_ip > 64
    assert _status(lambda: sd.op_ip_attention(z(1, 4, 96), z(1, 4, 96), z(1, 4, 96), z(1, 4, 96), one, 2))[0] == SDMI_ERR_UNSUPPORTED           # d_head 48
    assert _status(lambda: sd.op_ip_attention(z(1, 4, 160), z(1, 4, 160), z(1, 4, 160), z(1, 4, 160), one, 3))[0] == SDMI_ERR_INVALID           # 160 % 3
    if precision:
        assert _status(lambda: sd.op_ip_attention(z(1, 4, 160), z(1, 4, 160), z(1, 4, 160), z(1, 4, 160), one, 4, planes=True))[0] == SDMI_ERR_INVALID


# ---- the model-level contexts -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adapter(mc, cd):
    return syn.ip_adapter(mc, cd, D_EMB, T_IMG)


def _load(sd, ad, mc):
    layers = syn.ip_adapter_layers(mc)
    sd.set_ip_adapter_weights(ad["image_proj.proj.weight"], ad["image_proj.proj.bias"], ad["image_proj.norm.weight"], ad["image_proj.norm.bias"],
                              [ad[kk] for kk, _, _ in layers], [ad[kv] for _, kv, _ in layers])


@pytest.fixture(scope="module")
def sdc(tiny_dims, synth):
    """the module's fp32 context: the tiny model with a ControlNet beside it (cleared, it runs the plain model's launches) and NO adapter yet"""
    sd = _make(tiny_dims, control_hint_ch=3)
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture
def sd(sdc, tiny_dims):
    if not sdc.ip_adapter_ready:
        _load(sdc, _adapter(tiny_dims.model_channels, tiny_dims.ctx_dim), tiny_dims.model_channels)
    yield sdc
    sdc.set_ip_adapter(None)
    sdc.set_control(None)


def _inputs(d, n=N, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(3, d.ctx_dim)
    lat = np.stack([syn.initial_latent(70 + seed + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, lat


def _embeds(n_sets=N, n_img=1):
    return np.stack([syn.image_embeds(i, n_img, D_EMB) for i in range(n_sets)])          # [n_sets, n_img, D]


def _ref_tokens(ad, cd, embeds):
    """([n_sets, T_ip, cd] positive, the same shape of image_proj(0)) in float64"""
    pos = np.stack([IR.tokens_of(ad, e, cd) for e in embeds])
    neg = np.stack([IR.zero_tokens(ad, cd, embeds.shape[1]) for _ in embeds])
    return pos, neg


# ---- 2. image_proj and the hoisted K_ip / V_ip -----------------------------------------------------------------------------------------------------------------
def test_image_tokens_and_hoisted_kv(sd, tiny_dims):
    d = tiny_dims
    ad = _adapter(d.model_channels, d.ctx_dim)
    assert sd.ip_adapter_dims() == (D_EMB, T_IMG)
    e = np.concatenate([syn.image_embeds(5, 3, D_EMB), np.zeros((1, D_EMB), np.float32)])       # three pictures and a zero embedding
    got = sd.ip_image_tokens(e)
    ref = IR.image_proj(ad, e, d.ctx_dim)
    print(f"ip_image_tokens: max|d| / max(1, |ref|) = {np.abs(got - ref).max() / max(1.0, np.abs(ref).max()):.3e}")
    _check(got, ref, "ip_image_tokens", FP32_BAR)
    assert np.abs(got[3]).max() > 0.1, "image_proj(0) is the bias through the norm, not zero"
    # two pictures per set, two sets, a CFG pair of two images: rows = [neg, neg, set 0, set 1]
    emb = _embeds(N, 2)
    sd.set_ip_adapter(embeds=emb, scale=SCALE)
    assert sd.get_ip_adapter() == {"n_sets": N, "T_ip": 2 * T_IMG, "scale": pytest.approx(SCALE), "start": 0.0, "end": 1.0}
    pos, neg = _ref_tokens(ad, d.ctx_dim, emb)
    rows = np.concatenate([neg, pos])
    worst = 0.0
    for i, ((gk, gv), (rk, rv)) in enumerate(zip(sd.ip_kv(N, cfg_pair=True), IR.layer_kv(ad, d.model_channels, rows))):
        _check(gk, rk, f"K_ip of cross attention {i}", FP32_BAR)
        _check(gv, rv, f"V_ip of cross attention {i}", FP32_BAR)
        worst = max(worst, np.abs(gk - rk).max() / max(1.0, np.abs(rk).max()), np.abs(gv - rv).max() / max(1.0, np.abs(rv).max()))
    print(f"hoisted K_ip / V_ip: worst max|d| / max(1, |ref|) = {worst:.3e}")
    # one image more than sets: image 2 reads set 0 again; without a CFG pair every row is a conditional one
    kv3 = sd.ip_kv(3, cfg_pair=False)
    assert np.array_equal(_bits(kv3[0][0][2]), _bits(kv3[0][0][0])) and not np.array_equal(_bits(kv3[0][0][1]), _bits(kv3[0][0][0]))


@functools.lru_cache(maxsize=None)
def _synth():
    """one weight provider for every reference of the module: it keeps what it has generated"""
    return syn.SyntheticWeights(cache=True)


# ---- 3. model level -------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward_ref(wide: bool, dtype, on: bool, t=500):
    d = BF16_DIMS if wide else O.Dims(160, 4, 64, 16, 16, 32)
    ad = _adapter(d.model_channels, d.ctx_dim)
    ctx, _, lat = _inputs(d, seed=1)
    pos, _ = _ref_tokens(ad, d.ctx_dim, _embeds())
    unet = IR.IpUNetOracle(_synth(), d, dtype)
    return IR.ip_forward(unet, torch.from_numpy(lat), t, torch.from_numpy(ctx), (ad, pos, SCALE) if on else None).numpy()


def test_forward_fp32(sd, tiny_dims):
    """unet.forward with an adapter (no CFG pair: every row reads its positive tokens; the window does not apply) against the oracle with the image term in attn2"""
    d = tiny_dims
    assert d == O.Dims(160, 4, 64, 16, 16, 32)
    ctx, _, lat = _inputs(d, seed=1)
    plain = sd.unet.forward(lat, [500], ctx)
    k0 = sd.last_call_stats()["kernels"]
    sd.set_ip_adapter(embeds=_embeds(), scale=SCALE, start=0.5, end=0.5)
    got = sd.unet.forward(lat, [500], ctx)
    k1 = sd.last_call_stats()["kernels"]
    e64, e32 = _assert_close(got, _forward_ref(False, torch.float32, True), _forward_ref(False, torch.float64, True), "adapted forward")
    print(f"adapted forward: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.ip_kv(N)
    k_prep = sd.last_call_stats()["kernels"]      # the launches of the call's 32 K_ip / V_ip projections
    assert k_prep >= 32 and k1 - k0 == 16 + k_prep, "one launch per cross attention beside the per-call projections"
    assert np.abs(got - plain).max() > 1e-3, "the adapter does not reach the output"
    assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(got)), "two runs give different bits"
    e64, e32 = _assert_close(plain, _forward_ref(False, torch.float32, False), _forward_ref(False, torch.float64, False), "plain forward")


def _sample_refs(synth, d, ctx, unc, x, ts, step, window, embeds, control=None, neg=None):
    ad = _adapter(d.model_channels, d.ctx_dim)
    pos, zero = _ref_tokens(ad, d.ctx_dim, embeds)
    a = syn.alphas_cumprod()
    refs = []
    for dt in (torch.float32, torch.float64):
        c = None
        if control is not None:
            hint, strength = control
            c = (CR.ControlNetOracle(synth, d, dt), CR.hint01(hint), strength)
        pred = IR.IpPredictor(synth, d, dt, ad, pos, zero if neg is None else neg, SCALE, window[0], window[1], len(ts), control=c)
        refs.append(CR.sample(pred, a, ctx, unc, 7.5, ts, step, x(dt) if callable(x) else x).numpy())
    return refs


def test_sample_latent(sd, synth, tiny_dims):
    """4 steps; the conditional half reads the image tokens, the unconditional half image_proj(0); two pictures per image"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=3)
    emb = _embeds(N, 2)
    sd.set_ip_adapter(embeds=emb, scale=SCALE)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    ts, step = O.ddim_timesteps(4)
    refs = _sample_refs(synth, d, ctx, unc, lat, ts, step, (0.0, 1.0), emb)
    e64, e32 = _assert_close(got, refs[0], refs[1], "adapted sample_latent")
    print(f"adapted sample_latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.set_ip_adapter(None)
    assert np.abs(sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat) - got).max() > 1e-3


def test_sample_latent_first_half_window(sd, synth, tiny_dims):
    """start 0, end 0.5 of 4 steps: the adapter is on in steps 0 and 1, and the reference doing the same agrees"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=4)
    emb = _embeds()
    sd.set_ip_adapter(embeds=emb, scale=SCALE, start=0.0, end=0.5)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    ts, step = O.ddim_timesteps(4)
    assert CR.window(0.0, 0.5, 4) == [0, 1]
    refs = _sample_refs(synth, d, ctx, unc, lat, ts, step, (0.0, 0.5), emb)
    e64, e32 = _assert_close(got, refs[0], refs[1], "adapted sample_latent, window [0, 0.5)")
    print(f"adapted sample_latent, first half: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    sd.set_ip_adapter(embeds=emb, scale=SCALE)
    assert np.abs(sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat) - got).max() > 1e-4, "the window changes nothing"


def test_sample_latent_with_a_control(sd, synth, tiny_dims):
    """a controlled call: the UNet's cross attentions are adapted, the control encoder's are not"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=5)
    g = np.random.default_rng(905)
    hint = g.integers(0, 256, (N, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=np.uint8)
    hint[1] //= 4
    emb = _embeds()
    sd.set_control(hint, strength=0.6)
    sd.set_ip_adapter(embeds=emb, scale=SCALE)
    got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
    ts, step = O.ddim_timesteps(4)
    refs = _sample_refs(synth, d, ctx, unc, lat, ts, step, (0.0, 1.0), emb, control=(hint, 0.6))
    e64, e32 = _assert_close(got, refs[0], refs[1], "adapter + ControlNet sample_latent")
    print(f"adapter + ControlNet sample_latent: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


def test_sample_latent_from(sd, synth, tiny_dims):
    """img2img: the last 2 of 4 steps, the window counting the call's own steps"""
    d = tiny_dims
    ctx, unc, noise = _inputs(d, seed=6)
    z0 = (np.random.default_rng(6).standard_normal((N, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    emb = _embeds()
    sd.set_ip_adapter(embeds=emb, scale=SCALE, start=0.5, end=1.0)
    got = sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=noise)
    a = syn.alphas_cumprod()
    ts, step = R.timesteps(4, 0.5)
    assert len(ts) == 2 and CR.window(0.5, 1.0, 2) == [1]
    a0 = float(a[ts[0]])
    refs = _sample_refs(synth, d, ctx, unc, lambda dt: np.sqrt(a0) * torch.from_numpy(z0).to(dt) + np.sqrt(1.0 - a0) * torch.from_numpy(noise).to(dt), ts, step, (0.5, 1.0), emb)
    e64, e32 = _assert_close(got, refs[0], refs[1], "adapted img2img")
    print(f"adapted img2img: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")


@pytest.fixture(scope="module", params=[1, 2])
def sd_lowp(request, synth):
    """the wide model at precisions 1 and 2 with an adapter loaded and a ControlNet beside it (cleared, it runs the plain model's launches)"""
    sd = _make(BF16_DIMS, request.param, control_hint_ch=3)
    sd.load_weights(synth, clip=False)
    if request.param == 2:
        sd.set_option("fp8_min_rows", 1)     # 16 x 16 latents have few rows per GEMM: the MXFP8 path anyway (tests/test_fp8_gpu.py)
    _load(sd, _adapter(BF16_DIMS.model_channels, BF16_DIMS.ctx_dim), BF16_DIMS.model_channels)
    yield sd, request.param
    sd.close()


def test_forward_low_precision(sd_lowp):
    """relative RMS against the fp64 oracle, held to the plain forward's bars; the plain forward's figure on the same inputs is printed beside it"""
    sd, precision = sd_lowp
    ctx, _, lat = _inputs(BF16_DIMS, seed=1)
    bar = BAR_UNET if precision == 1 else BAR_UNET_FP8
    try:
        sd.set_ip_adapter(None)
        plain = sd.unet.forward(lat, [500], ctx)
        r_off = _rel_rms(plain, _forward_ref(True, torch.float64, False))
        sd.set_ip_adapter(embeds=_embeds(), scale=SCALE)
        got = sd.unet.forward(lat, [500], ctx)
        r_on = _rel_rms(got, _forward_ref(True, torch.float64, True))
        print(f"precision {precision} adapted forward: rel-RMS vs fp64 = {r_on:.3e} (adapter off, same inputs: {r_off:.3e}; bar {bar:.3e})")
        assert np.isfinite(got).all() and r_off < bar
        assert r_on < bar
        assert np.abs(got - plain).max() > 1e-3
        assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(got))
    finally:
        sd.set_ip_adapter(None)


def _wide_hint():
    g = np.random.default_rng(906)
    hint = g.integers(0, 256, (N, 8 * BF16_DIMS.latent_h, 8 * BF16_DIMS.latent_w, 3), dtype=np.uint8)
    hint[1] //= 4
    return hint


def _wide_z0():
    return (np.random.default_rng(16).standard_normal((N, 4, BF16_DIMS.latent_h, BF16_DIMS.latent_w)) * 0.8).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _sample_ref64_wide(on: bool, control: bool = False, img2img: bool = False):
    """the fp64 reference of a 4-step sample_latent -- img2img: of the last 2 of 4 steps from _wide_z0 -- with the adapter on or off, control: a ControlNet at 0.6"""
    d = BF16_DIMS
    synth = _synth()
    ctx, unc, lat = _inputs(d, seed=3)
    ad = _adapter(d.model_channels, d.ctx_dim)
    pos, zero = _ref_tokens(ad, d.ctx_dim, _embeds())
    a = syn.alphas_cumprod()
    if img2img:
        ts, step = R.timesteps(4, 0.5)
        a0 = float(a[ts[0]])
        x = np.sqrt(a0) * torch.from_numpy(_wide_z0()).to(torch.float64) + np.sqrt(1.0 - a0) * torch.from_numpy(lat).to(torch.float64)
    else:
        (ts, step), x = O.ddim_timesteps(4), lat
    c = (CR.ControlNetOracle(synth, d, torch.float64), CR.hint01(_wide_hint()), 0.6) if control else None
    pred = IR.IpPredictor(synth, d, torch.float64, ad, pos, zero, SCALE if on else 0.0, 0.0, 1.0, len(ts), control=c)
    return CR.sample(pred, a, ctx, unc, 7.5, ts, step, x).numpy()


@functools.lru_cache(maxsize=None)
def _controlled_forward_ref64_wide(on: bool, t=500):
    d = BF16_DIMS
    synth = _synth()
    ad = _adapter(d.model_channels, d.ctx_dim)
    ctx, _, lat = _inputs(d, seed=1)
    pos, _ = _ref_tokens(ad, d.ctx_dim, _embeds())
    x, c = torch.from_numpy(lat), torch.from_numpy(ctx)
    r = CR.ControlNetOracle(synth, d, torch.float64).forward(x, t, c, CR.hint01(_wide_hint()))
    return IR.ip_forward(IR.IpUNetOracle(synth, d, torch.float64), x, t, c, (ad, pos, SCALE) if on else None, r, 0.6).numpy()


def test_sample_latent_low_precision(sd_lowp):
    """a 4-step sample_latent against the fp64 reference, under the forward's bar; the same figure with the adapter off beside it"""
    sd, precision = sd_lowp
    ctx, unc, lat = _inputs(BF16_DIMS, seed=3)
    bar = BAR_UNET if precision == 1 else BAR_UNET_FP8
    try:
        sd.set_ip_adapter(None)
        r_off = _rel_rms(sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat), _sample_ref64_wide(False))
        sd.set_ip_adapter(embeds=_embeds(), scale=SCALE)
        got = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat)
        r_on = _rel_rms(got, _sample_ref64_wide(True))
        print(f"precision {precision} adapted 4-step sample_latent: rel-RMS vs fp64 = {r_on:.3e} (adapter off, same inputs: {r_off:.3e}; bar {bar:.3e})")
        assert np.isfinite(got).all()
        assert r_on < bar
    finally:
        sd.set_ip_adapter(None)


def _off_on(sd, precision, what, run, ref, off_ref=True):
    """rel-RMS of run() against ref(True) with the adapter on, under the plain forward's bar; off_ref: the figure with the adapter off against ref(False) is printed
    beside it (a sampled fp64 reference takes the CPU tens of seconds, so the sampled cases with a control and from an init latent do without).  The caller restores
    the state."""
    bar = BAR_UNET if precision == 1 else BAR_UNET_FP8
    sd.set_ip_adapter(None)
    plain = run()
    off = f"adapter off, same inputs: {_rel_rms(plain, ref(False)):.3e}; " if off_ref else ""
    sd.set_ip_adapter(embeds=_embeds(), scale=SCALE)
    got = run()
    r_on = _rel_rms(got, ref(True))
    print(f"precision {precision} {what}: rel-RMS vs fp64 = {r_on:.3e} ({off}bar {bar:.3e})")
    assert np.isfinite(got).all()
    assert r_on < bar
    assert np.abs(got - plain).max() > 1e-3, f"{what}: the adapter does not reach the output"


def test_forward_with_a_control_low_precision(sd_lowp):
    """the adapted forward of a controlled context: in the fp8_linear block the image term is added in front of the quantisation, the control's residuals after it"""
    sd, precision = sd_lowp
    ctx, _, lat = _inputs(BF16_DIMS, seed=1)
    try:
        sd.set_control(_wide_hint(), strength=0.6)
        _off_on(sd, precision, "adapter + ControlNet forward", lambda: sd.unet.forward(lat, [500], ctx), _controlled_forward_ref64_wide)
    finally:
        sd.set_ip_adapter(None)
        sd.set_control(None)


def test_sample_latent_with_a_control_low_precision(sd_lowp):
    sd, precision = sd_lowp
    ctx, unc, lat = _inputs(BF16_DIMS, seed=3)
    try:
        sd.set_control(_wide_hint(), strength=0.6)
        _off_on(sd, precision, "adapter + ControlNet 4-step sample_latent", lambda: sd.sample_latent(ctx, unc, 7.5, 4, init_latent=lat),
                lambda on: _sample_ref64_wide(on, control=True), off_ref=False)
    finally:
        sd.set_ip_adapter(None)
        sd.set_control(None)


def test_sample_latent_from_low_precision(sd_lowp):
    """img2img: the last 2 of 4 steps"""
    sd, precision = sd_lowp
    ctx, unc, noise = _inputs(BF16_DIMS, seed=3)
    try:
        _off_on(sd, precision, "adapted img2img", lambda: sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, _wide_z0(), noise=noise),
                lambda on: _sample_ref64_wide(on, img2img=True), off_ref=False)
    finally:
        sd.set_ip_adapter(None)


# ---- 4. off means off -----------------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(sdc, sd_tiny, tiny_dims):
    """no adapter, a cleared setting, scale 0, a window without a step: the bits and the launch count of a context that never heard of an adapter"""
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=7)
    sd_tiny.set_latent_size(d.latent_h, d.latent_w)
    want = sd_tiny.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    k_want = sd_tiny.last_call_stats()["kernels"]
    want_f = sd_tiny.unet.forward(lat, [500], ctx)
    kf_want = sd_tiny.last_call_stats()["kernels"]
    sdc.set_ip_adapter(None)
    sdc.set_control(None)
    emb = _embeds()

    def same(name):
        got = sdc.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
        assert np.array_equal(_bits(got), _bits(want)), name
        assert sdc.last_call_stats()["kernels"] == k_want, name

    sdc.clear_ip_adapter_weights()
    assert not sdc.ip_adapter_ready
    same("no adapter loaded")
    assert _status(lambda: sdc.set_ip_adapter(tokens=np.zeros((1, 4, d.ctx_dim), np.float32)))[0] == SDMI_ERR_STATE
    assert _status(lambda: sdc.ip_image_tokens(np.zeros((1, D_EMB), np.float32)))[0] == SDMI_ERR_STATE
    assert sdc.get_ip_adapter() is None
    _load(sdc, _adapter(d.model_channels, d.ctx_dim), d.model_channels)
    same("loaded, not set")
    try:
        states = {"cleared": lambda: sdc.set_ip_adapter(None), "scale 0": lambda: sdc.set_ip_adapter(embeds=emb, scale=0.0),
                  "empty window": lambda: sdc.set_ip_adapter(embeds=emb, scale=SCALE, start=0.4, end=0.4),
                  "window past the last step": lambda: sdc.set_ip_adapter(embeds=emb, scale=SCALE, start=1.0, end=1.0)}
        for name, setter in states.items():
            sdc.set_ip_adapter(embeds=emb, scale=SCALE)      # from a state that is on
            assert np.abs(sdc.sample_latent(ctx, unc, 7.5, 3, init_latent=lat) - want).max() > 1e-3
            setter()
            same(name)
            assert np.array_equal(_bits(sdc.unet.forward(lat, [500], ctx)), _bits(want_f)) == (name in ("cleared", "scale 0")), name     # (unet.forward has no window)
            if name in ("cleared", "scale 0"):
                assert sdc.last_call_stats()["kernels"] == kf_want, name
    finally:
        sdc.set_ip_adapter(None)


def test_refusals_keep_the_state(sd, tiny_dims):
    d = tiny_dims
    ctx, _, lat = _inputs(d, seed=8)
    emb = _embeds()
    sd.set_ip_adapter(embeds=emb, scale=SCALE, start=0.25, end=0.75)
    state = sd.get_ip_adapter()
    want = sd.unet.forward(lat, [500], ctx)
    bad = [dict(embeds=emb, scale=float("nan")), dict(embeds=emb, start=0.6, end=0.5), dict(embeds=emb, end=1.5), dict(embeds=np.zeros((1, 1, D_EMB + 32), np.float32)),
           dict(tokens=np.zeros((1, 4, d.ctx_dim + 1), np.float32)), dict(embeds=emb, negative_tokens=np.zeros((N, T_IMG, d.ctx_dim + 1), np.float32))]
    for kw in bad:
        st, msg = _status(lambda: sd.set_ip_adapter(**kw))
        assert st == SDMI_ERR_INVALID and "ip_adapter" in msg, (kw.keys(), st, msg)
        assert sd.get_ip_adapter() == state, "a refused setting changed the state"
    st, msg = _status(lambda: sd.set_ip_adapter(tokens=np.zeros((1, 65, d.ctx_dim), np.float32)))
    assert st == SDMI_ERR_UNSUPPORTED and sd.get_ip_adapter() == state
    assert np.array_equal(_bits(sd.unet.forward(lat, [500], ctx)), _bits(want)), "the earlier setting is no longer in force"


# ---- 5. loading ---------------------------------------------------------------------------------------------------------------------------------------------
def test_fp16_file_gives_the_bits_of_the_widened_arrays(sd, tiny_dims, tmp_path):
    d = tiny_dims
    ad = _adapter(d.model_channels, d.ctx_dim)
    ctx, unc, lat = _inputs(d, seed=9)
    emb = _embeds()
    try:
        for dtype, widen in (("F16", lambda a: a.astype(np.float16).astype(np.float32)), ("BF16", bf16_round)):
            path = tmp_path / f"ip_{dtype}.safetensors"
            write_ip_adapter_safetensors(path, ad, dtype)
            sd.load_ip_adapter_safetensors(path)
            assert sd.ip_adapter_ready and sd.get_ip_adapter() is None, "loading an adapter clears the setting made for the old one"
            sd.set_ip_adapter(embeds=emb, scale=SCALE)
            from_file = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
            _load(sd, {k: widen(a) for k, a in ad.items()}, d.model_channels)
            sd.set_ip_adapter(embeds=emb, scale=SCALE)
            assert np.array_equal(_bits(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)), _bits(from_file)), dtype
        # a refused file leaves the adapter in force
        bad = {k: v for k, v in ad.items() if k != "ip_adapter.7.to_v_ip.weight"}
        write_ip_adapter_safetensors(tmp_path / "bad.safetensors", bad, "F16")
        st, msg = _status(lambda: sd.load_ip_adapter_safetensors(tmp_path / "bad.safetensors"))
        assert st == -3 and "'ip_adapter.7.to_v_ip.weight'" in msg
        assert np.array_equal(_bits(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)), _bits(from_file))
    finally:
        _load(sd, ad, d.model_channels)


def test_embeds_file_gives_the_bits_of_the_widened_array(sd, tiny_dims, tmp_path):
    """sdmi_set_ip_adapter_file, the command line's route: "image_embeds" [n, D] as F32 / F16 / BF16 -- subnormal, zero and negative halves among them -- is the
    setting set_ip_adapter makes of the widened array"""
    d = tiny_dims
    e = syn.image_embeds(7, 2, D_EMB)
    e[0, :6] = [0.0, -0.0, 6.0e-8, -3.1e-5, 6.1e-5, 65504.0]        # in half: zeros, the smallest subnormal, a subnormal, the smallest normal, the largest
    e[1, :3] = [-2.0e-7, 1.0e-3, -1.0]
    from stable_diffusion_burn_amd.weights import bf16_bits, write_safetensors
    forms = {"F32": (e, e), "F16": (e.astype(np.float16), e.astype(np.float16).astype(np.float32)), "BF16": ((bf16_bits(e).reshape(e.shape), "BF16"), bf16_round(e))}
    for tag, (stored, widened) in forms.items():
        path = tmp_path / f"embeds_{tag}.safetensors"
        write_safetensors(path, {"image_embeds": stored})
        sd.set_ip_adapter(embeds=widened, scale=SCALE, start=0.25, end=0.75)
        want_state, want = sd.get_ip_adapter(), sd.ip_kv(1)
        assert want_state["T_ip"] == 2 * T_IMG
        sd.set_ip_adapter(None)
        sd.set_ip_adapter_file(path, scale=SCALE, start=0.25, end=0.75)
        assert sd.get_ip_adapter() == want_state, tag
        for i, ((gk, gv), (wk, wv)) in enumerate(zip(sd.ip_kv(1), want)):
            assert np.array_equal(_bits(gk), _bits(wk)) and np.array_equal(_bits(gv), _bits(wv)), f"{tag}: K_ip / V_ip of cross attention {i}"
    state = sd.get_ip_adapter()
    write_safetensors(tmp_path / "other.safetensors", {"embeds": e})
    write_safetensors(tmp_path / "narrow.safetensors", {"image_embeds": e[:, :32]})
    write_safetensors(tmp_path / "many.safetensors", {"image_embeds": np.zeros((17, D_EMB), np.float32)})
    assert _status(lambda: sd.set_ip_adapter_file(tmp_path / "other.safetensors"))[0] == -3
    assert _status(lambda: sd.set_ip_adapter_file(tmp_path / "narrow.safetensors"))[0] == SDMI_ERR_INVALID
    assert _status(lambda: sd.set_ip_adapter_file(tmp_path / "many.safetensors"))[0] == SDMI_ERR_UNSUPPORTED
    assert sd.get_ip_adapter() == state, "a refused file changed the setting"


def test_explicit_negative_tokens_reproduce_the_default(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=10)
    emb = _embeds(N, 2)
    sd.set_ip_adapter(embeds=emb, scale=SCALE)
    want = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)
    # projected outside, in the calls the setting itself makes (all pictures of all sets at once; one zero embedding, repeated per picture), passed as tokens
    tokens = sd.ip_image_tokens(emb.reshape(-1, D_EMB)).reshape(N, 2 * T_IMG, d.ctx_dim)
    zero = np.tile(sd.ip_image_tokens(np.zeros((1, D_EMB), np.float32)), (N, 2, 1))
    sd.set_ip_adapter(tokens=tokens, negative_tokens=zero, scale=SCALE)
    assert np.array_equal(_bits(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)), _bits(want))
    sd.set_ip_adapter(tokens=tokens, negative_tokens=tokens, scale=SCALE)
    assert not np.array_equal(_bits(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=lat)), _bits(want)), "the negative tokens are not read"


# ---- 6. scratch independence, the sharded call -----------------------------------------------------------------------------------------------------------------
def test_scratch_fill(sd, tiny_dims, tmp_path):
    d = tiny_dims
    ctx, unc, lat = _inputs(d, seed=11)
    sd.set_ip_adapter(embeds=_embeds(N, 2), scale=SCALE)
    _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), "adapted unet.forward")


def test_scratch_fill_low_precision(sd_lowp, tmp_path):
    sd, precision = sd_lowp
    ctx, unc, lat = _inputs(BF16_DIMS, seed=11)
    try:
        sd.set_ip_adapter(embeds=_embeds(), scale=SCALE)
        _sweep(sd, tmp_path, lambda: sd.unet.forward(lat, [500], ctx), f"adapted unet.forward precision {precision}")
    finally:
        sd.set_ip_adapter(None)


def test_sharded_call_gives_the_single_contexts_bits(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    d = tiny_dims
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=(0,))
    try:
        m.load_weights(synth)
        _load(m.device_view(0), _adapter(d.model_channels, d.ctx_dim), d.model_channels)
        n = 3
        lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(n)])
        ctx, unc = syn.cond_context(0, T, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        plain = m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat)
        emb = _embeds(1, 1)
        m.set_ip_adapter(embeds=emb, scale=SCALE)
        sd.set_ip_adapter(embeds=emb, scale=SCALE)
        got = m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat)
        ref = sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 2, init_latent=lat)
        assert np.array_equal(got, ref)
        assert (got != plain).any(), "the adapter does not reach the sharded call"
        # a refusal leaves the setting in force: the arguments, then the adapter's dims, are checked on every device before any takes the setting
        assert _status(lambda: m.set_ip_adapter(embeds=np.zeros((1, 1, D_EMB + 32), np.float32)))[0] == SDMI_ERR_INVALID
        assert np.array_equal(m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat), got)
        m.set_ip_adapter(None)
        assert np.array_equal(m.sample_image(ctx, unc, 7.5, 2, n, init_latents=lat), plain)
        m.device_view(0).clear_ip_adapter_weights()
        assert _status(lambda: m.set_ip_adapter(embeds=emb, scale=SCALE))[0] == SDMI_ERR_STATE
    finally:
        m.close()
