"""CFG rescale and zero-terminal-SNR schedules through the sampling entries (include/sdmi.h "CFG rescale and zero-terminal-SNR schedules"):
tiny dims, 4 steps, fp32, against the oracle with the rescale hook (tests/guidance_ref.py) driven by the textbook loops of sampler_ref / ksampler_ref /
zero_snr_ref.  Bars are test_sampler_gpu.py's: |gpu - f64| <= max(1e-3, 2 |f32 - f64|)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import guidance_ref as G
import img2img_ref as R
import ksampler_ref as K
import sampler_ref as S
import zero_snr_ref as Z
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_UNSUPPORTED = -1, -5
BAR_LATENT_BF16 = 2.6e-2   # tests/test_bf16_gpu.py: 5-step CFG latent at precision 1
NOISE_SEED = 0x5EED
PHI = 0.7
STEPS = 4
# (set_sampler kind, eta) or ("k", kind, schedule, eta)
CASES = [("default",), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("plms", 0.0), ("k", "heun", "karras", 0.0), ("k", "dpmpp_sde", "karras", 1.0)]
F = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731


def _reset(s):
    s.set_sampler(None)
    s.set_prediction("eps")
    s.set_guidance_rescale(0.0)
    s.set_zero_snr(False)


@pytest.fixture
def sd(sd_tiny):
    """the session's engine; whatever a test sets, the next test (of any file) finds the defaults"""
    _reset(sd_tiny)
    yield sd_tiny
    _reset(sd_tiny)


def _new_sd(d, synth, precision=0, vae_encoder=False, **kw):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    s = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision, **kw))
    s.load_weights(synth, clip=False, vae_encoder=vae_encoder)
    return s


def _assert_close(got, ref32, ref64, what, atol=1e-3):
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, ref32, ref64))
    assert np.isfinite(got).all(), f"{what}: non-finite"
    e64, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    bound = max(atol, 2 * e32)
    print(f"{what}: max|gpu-f64|={e64:.3e}  |f32-f64|={e32:.3e}  bound {bound:.3e}")
    assert e64 <= bound, f"{what}: max|gpu-f64|={e64:.3e} > {bound:.3e} (|f32-f64|={e32:.3e})"


def _inputs(d, n, T, Tu, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(Tu, d.ctx_dim)
    rng = np.random.default_rng(900 + seed)
    z0 = (rng.standard_normal((n, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    noise = np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, z0, noise


def _half_mask(n, h, w):
    m = np.zeros((n, 1, h, w), np.float32)
    m[..., : w // 2 - 1] = 1.0
    m[..., w // 2 - 1] = 0.75
    m[..., w // 2] = 0.25
    return m


def _oracles(synth, d, prediction, phi, alphas=None, **kw):
    a = syn.alphas_cumprod() if alphas is None else alphas
    return [G.GuidanceOracle(synth, a, d, dt, prediction, phi, **kw) for dt in (torch.float32, torch.float64)]


def _set(s, case):
    if case[0] == "default":
        s.set_sampler(None)
    elif case[0] == "k":
        s.set_ksampler(case[1], schedule=case[2], eta=case[3], noise_seed=NOISE_SEED)
    else:
        s.set_sampler(case[0], eta=case[1], noise_seed=NOISE_SEED)


def _ref_txt2img(ora, case, ctx, unc, n_steps, x_T, image_base=0):
    if case[0] == "k":
        sg = K.sigmas(case[2], ora.alphas, n_steps)
        return K.sample_latent(ora, ctx, unc, 7.5, sg, 0, x_T, case[1], case[3], NOISE_SEED, image_base)
    kind, eta = ("ddim", 0.0) if case[0] == "default" else case
    ts, step = O.ddim_timesteps(n_steps, ora.n_steps)
    return S.sample_latent(ora, ctx, unc, 7.5, ts, step, x_T, kind, eta, NOISE_SEED, image_base)


# ---- 1. fp32 parity with phi = 0.7 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["eps", "v"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_txt2img_parity(sd, synth, tiny_dims, case, prediction):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 2, 7, 3)
    sd.set_prediction(prediction)
    _set(sd, case)
    plain = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    sd.set_guidance_rescale(PHI)
    got = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    o32, o64 = _oracles(synth, d, prediction, PHI)
    r32 = _ref_txt2img(o32, case, ctx, unc, STEPS, x_T).numpy()
    r64 = _ref_txt2img(o64, case, ctx, unc, STEPS, x_T).numpy()
    _assert_close(got, r32, r64, f"txt2img {case} {prediction} phi={PHI}")
    print(f"largest factor of the run: {o64.max_f:.4f}; max|rescaled - plain| = {np.abs(got - plain).max():.3e}")
    assert np.abs(got - plain).max() > 1e-2   # and it is not the result without the rescale


@pytest.mark.parametrize("masked", [False, True])
def test_img2img_parity(sd, synth, tiny_dims, masked):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 5, 2, seed=1)
    mask = _half_mask(2, d.latent_h, d.latent_w) if masked else None
    for case in (("default",), ("dpmpp_2m", 0.0)):
        _set(sd, case)
        sd.set_guidance_rescale(PHI)
        got = sd.sample_latent_from(ctx, unc, 7.5, 5, 0.6, z0, mask=mask, noise=noise)
        kind, eta = ("ddim", 0.0) if case[0] == "default" else case
        refs = []
        for ora in _oracles(synth, d, "eps", PHI):
            ts, step = R.timesteps(5, 0.6, ora.n_steps)
            a0 = float(ora.alphas[ts[0]])
            z0_, eps_ = torch.as_tensor(z0).to(ora.dtype), torch.as_tensor(noise).to(ora.dtype)
            x = math.sqrt(a0) * z0_ + math.sqrt(1.0 - a0) * eps_
            refs.append(S.sample_latent(ora, ctx, unc, 7.5, ts, step, x, kind, eta, NOISE_SEED, 0, mask, z0_ if masked else None, eps_ if masked else None).numpy())
        _assert_close(got, refs[0], refs[1], f"img2img {case} masked={masked} phi={PHI}")
        if masked:
            assert np.array_equal(got[..., -1], z0[..., -1])


def test_cond_parity(synth, tiny_dims):
    """one _cond call on an unet_in_ch = 9 context: the rescale sits behind the conditioned forwards like behind any other"""
    import inpaint_ref as IR
    d = tiny_dims
    s = _new_sd(d, synth, unet_in_ch=9)
    try:
        ctx, unc, z0, noise = _inputs(d, 2, 7, 3, seed=2)
        cond = np.random.default_rng(5).standard_normal((2, 5, d.latent_h, d.latent_w)).astype(np.float32)
        cond[:, 0] = cond[:, 0] > 0
        s.set_guidance_rescale(PHI)
        got = s.sample_latent_from(ctx, unc, 7.5, STEPS, 1.0, z0, noise=noise, cond=cond)
        refs = []
        for dt in (torch.float32, torch.float64):
            ora = G.GuidanceOracle(synth, syn.alphas_cumprod(), d, dt, "eps", PHI, unet=IR.CondUNetOracle(synth, d, dt, 9), cond=cond)
            ts, step = R.timesteps(STEPS, 1.0, ora.n_steps)
            a0 = float(ora.alphas[ts[0]])
            x = math.sqrt(a0) * torch.as_tensor(z0).to(dt) + math.sqrt(1.0 - a0) * torch.as_tensor(noise).to(dt)
            refs.append(S.sample_latent(ora, ctx, unc, 7.5, ts, step, x, "ddim").numpy())
        _assert_close(got, refs[0], refs[1], f"img2img_latent_cond phi={PHI}")
    finally:
        s.close()


# ---- 2. one launch per evaluation, the same classes -------------------------------------------------------------------------------------------
def test_one_update_launch_per_evaluation(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 1, 7, 2, seed=3)
    mask = _half_mask(1, d.latent_h, d.latent_w)
    for case in CASES:
        _set(sd, case)
        stats = {}
        for phi in (0.0, PHI):
            sd.set_guidance_rescale(phi)
            sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise)
            a = sd.last_call_stats()["kernels"]
            sd.sample_latent_from(ctx, unc, 7.5, 5, 1.0, z0, mask=mask, noise=noise)
            b = sd.last_call_stats()["kernels"]
            try:
                sd.set_option("profile", 1)
                sd.set_option("profile_reset", 1)
                sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise)
                prof = {k: v["launches"] for k, v in sd.profile_stats().items()}
            finally:
                sd.set_option("profile", 0)
            stats[phi] = (a, b, prof)
        print(case, stats[PHI][:2], stats[PHI][2]["other"])
        assert stats[0.0] == stats[PHI], case


# ---- 3. phi = 0 is the path it was ------------------------------------------------------------------------------------------------------------
def test_phi_0_is_untouched(sd, synth, tiny_dims):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 7, 3, seed=4)
    mask = _half_mask(2, d.latent_h, d.latent_w)
    cases = [("default",), ("dpmpp_2m", 0.0), ("k", "dpmpp_2m", "karras", 0.0)]

    def calls(s, case):
        _set(s, case)
        out = []
        for f in (lambda: s.sample_latent(ctx, unc, 7.5, STEPS, init_latent=noise),
                  lambda: s.sample_latent_from(ctx, unc, 7.5, STEPS, 0.75, z0, mask=mask, noise=noise)):
            out.append((f(), s.last_call_stats()["kernels"]))
        return out

    fresh = _new_sd(d, synth)
    try:
        ref = {c: calls(fresh, c) for c in cases}
    finally:
        fresh.close()
    for c in cases:
        sd.set_guidance_rescale(PHI)
        on = calls(sd, c)
        sd.set_guidance_rescale(0.0)
        for (a, ka), (b, kb), (r, _) in zip(calls(sd, c), ref[c], on):
            assert np.array_equal(a, b) and ka == kb, c
            assert not np.array_equal(a, r), c


def test_invalid_phi_is_refused(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 1, 7, 2, seed=5)
    sd.set_guidance_rescale(PHI)
    want = sd.sample_latent(ctx, unc, 7.5, 2, init_latent=x_T)
    for phi in (-0.01, 1.0001, float("nan"), float("inf")):
        assert sd._lib.sdmi_set_guidance_rescale(sd._ctx, phi) == SDMI_ERR_INVALID, phi
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, 2, init_latent=x_T), want)   # the value in force stayed
    for phi in (0.0, 1.0):
        sd.set_guidance_rescale(phi)


# ---- 4. batch and sharding ------------------------------------------------------------------------------------------------------------------
# The UNet plans its launches for the batch it is given: split-K and tile per GEMM shape (the row count is n * hw), key slices of the fp32 attention, the paired and
# folded launches of sections 4b / 4c, the layers shared between the CFG halves, and how many workgroups share a GroupNorm sample.  Each changes the order of fp32 sums, so
# at the default options a batch and its single calls agree to a few ulps only (test_sampler_gpu.py's twin of the test below allows 2e-5 * max|x|; measured here at 4
# steps, DDIM eta = 1: 1.6 .. 2.1e-4 at phi = 0, 0.9 .. 1.2e-4 at phi = 0.7, on latents of magnitude 60).  With those plans pinned by the engine options that exist for
# such tests, every launch computes an image the same way at any batch size, and what is left to differ is what this feature adds.
PINNED_PLANS = {"splitk": 1, "gemm_tile": 0, "attn_kv_splits": 1, "skip_slices": 0, "proj_out_fold": 0, "ups_phase": 0, "cfg_share": 0, "geglu_fuse": 0,
                "gn32_min_wgs": 1, "gn32_stats_min_wgs": 1, "gn_target_wgs": 1}


@pytest.fixture(scope="module")
def sd_pinned(tiny_dims, synth):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    d = tiny_dims
    s = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch))
    for k, v in PINNED_PLANS.items():
        s.set_option(k, v)
    s.load_weights(synth, clip=False, vae_encoder=False)
    yield s
    s.close()


@pytest.mark.parametrize("case", [("ddim", 1.0), ("dpmpp_2m", 0.0)], ids=lambda c: c[0])
def test_batch_equals_single_calls_with_image_base(sd_pinned, tiny_dims, case):
    """a batch of 3 against three single calls with image_base under phi = 0.7, bit for bit, eta = 1 included -- and the same at phi = 0, which shows that the pinned
    engine is batch-invariant to begin with and that the rescale kernel keeps it so"""
    d, sd = tiny_dims, sd_pinned
    ctx, unc, _, x_T = _inputs(d, 3, 7, 2, seed=6)
    try:
        for phi in (0.0, PHI):
            sd.set_guidance_rescale(phi)
            sd.set_sampler(case[0], eta=case[1], noise_seed=NOISE_SEED)
            batch = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
            for i in range(3):
                sd.set_sampler(case[0], eta=case[1], noise_seed=NOISE_SEED, image_base=i)
                one = sd.sample_latent(ctx[i:i + 1], unc, 7.5, STEPS, init_latent=x_T[i:i + 1])
                print(f"{case} phi = {phi} image {i}: batch vs single max|d| = {np.abs(batch[i:i + 1] - one).max():.2e}")
                assert np.array_equal(batch[i:i + 1], one), f"phi = {phi}, image {i}"
                if i == 1 and case[1] != 0.0:   # the base matters: image 1 with image 0's noise is another image
                    sd.set_sampler(case[0], eta=case[1], noise_seed=NOISE_SEED, image_base=0)
                    assert np.abs(batch[1:2] - sd.sample_latent(ctx[1:2], unc, 7.5, STEPS, init_latent=x_T[1:2])).max() > 1e-2
            if phi:
                sd.set_guidance_rescale(0.0)
                sd.set_sampler(case[0], eta=case[1], noise_seed=NOISE_SEED)
                assert not np.array_equal(sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T), batch)   # (the rescale was on)
    finally:
        sd.set_guidance_rescale(0.0)
        sd.set_sampler(None)


def test_multi_context_with_one_device_equals_single(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    d = tiny_dims
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=(0,))
    try:
        m.load_weights(synth)
        n = 3
        lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(n)])
        ctx, unc = syn.cond_context(0, 7, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        plain = m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat)
        m.set_guidance_rescale(PHI)
        sd.set_guidance_rescale(PHI)
        for kind, eta in (("ddim", 1.0), ("dpmpp_2m", 0.0)):
            m.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
            sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
            got = m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat)
            ref = sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 3, init_latent=lat)
            assert np.array_equal(got, ref), kind
        m.set_sampler(None)
        sd.set_sampler(None)
        got = m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat)
        assert np.array_equal(got, sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 3, init_latent=lat))
        assert not np.array_equal(got, plain)
        assert m._lib.sdmi_multi_set_guidance_rescale(m._m, 1.5) == SDMI_ERR_INVALID
        m.set_guidance_rescale(0.0)
        assert np.array_equal(m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat), plain)
    finally:
        m.close()


# ---- 5. zero terminal SNR end to end ----------------------------------------------------------------------------------------------------------
def _ref_zero_snr(ora, kind, eta, ctx, unc, ts, step, x, mask=None, z0=None, eps=None):
    dt = ora.dtype
    x = torch.as_tensor(x).to(dt)
    c, u = torch.as_tensor(ctx).to(dt), torch.as_tensor(unc).to(dt)
    n, _, h, w = x.shape
    predict_v = lambda x_, t, cur: ora.guided(x_, t, c, u, 7.5)                                           # noqa: E731
    noise = lambda s: torch.from_numpy(S.step_noise(NOISE_SEED, 0, n, s, h, w)).to(dt)                   # noqa: E731
    blend = None
    if mask is not None:
        m = torch.as_tensor(mask).to(dt).reshape(n, 1, h, w)
        z0_, eps_ = torch.as_tensor(z0).to(dt), torch.as_tensor(eps).to(dt)
        blend = lambda x_, prev: m * x_ + (1.0 - m) * (math.sqrt(prev) * z0_ + math.sqrt(1.0 - prev) * eps_)   # noqa: E731
    with torch.no_grad():
        return Z.sample_x0_eps(kind, eta, ora.alphas, ts, step, x, predict_v, noise, blend)


def test_zero_snr_schedule_state(sd):
    from stable_diffusion_burn_amd import rescale_zero_snr
    loaded = sd.schedule()
    assert np.array_equal(loaded, syn.alphas_cumprod())
    sd.set_zero_snr(True)
    zt = sd.schedule()
    assert zt[-1] == 0.0 and zt[0] == loaded[0] and np.array_equal(zt, rescale_zero_snr(loaded))
    sd.set_zero_snr(True)   # idempotent: the rescale is of the loaded table, not of the one in force
    assert np.array_equal(sd.schedule(), zt)
    sd.set_zero_snr(False)
    assert sd.schedule().tobytes() == loaded.tobytes()


@pytest.mark.parametrize("phi", [0.0, PHI])
@pytest.mark.parametrize("kind,eta", [("default", 0.0), ("ddim", 0.0), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("plms", 0.0)])
def test_zero_snr_txt2img_parity(sd, synth, tiny_dims, kind, eta, phi):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 2, 7, 3, seed=7)
    sd.set_zero_snr(True)
    sd.set_prediction("v")
    sd.set_guidance_rescale(phi)
    if kind != "default":
        sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
    zt = sd.schedule()
    assert zt[-1] == 0.0
    got = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    ts, step = O.ddim_timesteps(STEPS, len(zt))
    refs = [_ref_zero_snr(ora, "ddim" if kind == "default" else kind, eta, ctx, unc, ts, step, x_T).numpy() for ora in _oracles(synth, d, "v", phi, zt)]
    _assert_close(got, refs[0], refs[1], f"zero-SNR txt2img {kind} eta={eta} phi={phi}")


@pytest.mark.parametrize("strength,masked", [(1.0, False), (1.0, True), (0.5, False)])
def test_zero_snr_img2img_parity(sd, synth, tiny_dims, strength, masked):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 5, 2, seed=8)
    mask = _half_mask(2, d.latent_h, d.latent_w) if masked else None
    sd.set_zero_snr(True)
    sd.set_prediction("v")
    sd.set_guidance_rescale(PHI)
    sd.set_sampler("dpmpp_2m")
    zt = sd.schedule()
    got = sd.sample_latent_from(ctx, unc, 7.5, STEPS, strength, z0, mask=mask, noise=noise)
    ts, step = R.timesteps(STEPS, strength, len(zt))
    a0 = float(zt[ts[0]])
    assert (a0 == 0.0) == (strength == 1.0)
    x = math.sqrt(a0) * z0.astype(np.float64) + math.sqrt(1.0 - a0) * noise.astype(np.float64)   # strength 1: x = the noise
    refs = [_ref_zero_snr(ora, "dpmpp_2m", 0.0, ctx, unc, ts, step, x, mask, z0, noise).numpy() for ora in _oracles(synth, d, "v", PHI, zt)]
    _assert_close(got, refs[0], refs[1], f"zero-SNR img2img strength={strength} masked={masked}")


def test_zero_snr_refusals_and_restore(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd import SdmiError
    d = tiny_dims
    ctx, unc, z0, x_T = _inputs(d, 1, 7, 2, seed=9)
    out = np.empty_like(x_T)
    before = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    sd.set_prediction("v")
    before_v = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    sd.set_zero_snr(True)
    good = sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
    assert np.isfinite(good).all() and not np.array_equal(good, before_v)

    def launches():
        return sum(v["launches"] for v in sd.profile_stats().values())

    def refused(status, what):
        """20 refused calls of each sampling entry: the status, no launch, and (the pool returned) the good call's bits afterwards"""
        lib = sd._lib
        n0 = launches()
        for _ in range(20):
            assert lib.sdmi_sample_latent(sd._ctx, F(ctx), 1, 7, F(unc), 2, 7.5, STEPS, F(x_T), 0, F(out)) == status, what
            assert lib.sdmi_img2img_latent(sd._ctx, F(ctx), 1, 7, F(unc), 2, 7.5, STEPS, 0.5, F(z0), None, F(x_T), 0, F(out)) == status, what
        assert launches() == n0, what

    try:
        sd.set_option("profile", 1)
        sd.set_option("profile_reset", 1)
        sd.set_prediction("eps")
        for case in (("default",), ("ddim", 1.0), ("dpmpp_2m", 0.0), ("plms", 0.0)):
            _set(sd, case)
            refused(SDMI_ERR_INVALID, case)
        with pytest.raises(SdmiError) as e:
            sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T)
        assert "x0" in str(e.value)
        sd.set_prediction("v")
        sd.set_sampler(None)
        # a k-sampler: refused at set time on such a table ...
        with pytest.raises(SdmiError) as e:
            sd.set_ksampler("heun", schedule="karras")
        assert e.value.status == SDMI_ERR_UNSUPPORTED
        assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T), good)   # the context stayed as it was
        # ... and by the sampling call where the table came last
        sd.set_zero_snr(False)
        sd.set_ksampler("heun", schedule="karras")
        sd.set_zero_snr(True)
        refused(SDMI_ERR_UNSUPPORTED, "k-sampler")
        assert sd.get_ksampler() is not None
    finally:
        sd.set_option("profile", 0)
    sd.set_sampler(None)
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T), good)
    sd.set_zero_snr(False)
    assert sd.schedule().tobytes() == syn.alphas_cumprod().tobytes()
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T), before_v)
    sd.set_prediction("eps")
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, STEPS, init_latent=x_T), before)


def test_zero_snr_before_the_weights(synth, tiny_dims):
    """sticky, before or after any loader"""
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion, rescale_zero_snr
    d = tiny_dims
    s = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch))
    try:
        s.set_zero_snr(True)
        s.load_weights(synth, clip=False, vae_encoder=False)
        assert np.array_equal(s.schedule(), rescale_zero_snr(syn.alphas_cumprod()))
        s.set_zero_snr(False)
        assert np.array_equal(s.schedule(), syn.alphas_cumprod())
    finally:
        s.close()


# ---- 6. precision 1 ---------------------------------------------------------------------------------------------------------------------------
def test_precision_1(synth):
    """bf16 (dims as test_sampler_gpu.py::test_precision_1, 5 steps): the rel-RMS of the phi = 0.7 latent against the fp64 restatement of the same sampler, next to
    the phi = 0 arm measured here.  f_b multiplies the guided output -- and with it its bf16 error -- so the bar is the phi = 0 arm's own error times the largest f_b
    of the run, plus the project's 2.6e-2 floor."""
    d = O.Dims(320, 8, 768, 8, 8, 64)
    s = _new_sd(d, synth, precision=1)
    try:
        ctx, unc, _, x_T = _inputs(d, 1, 77, 77, seed=10)
        r, max_f = {}, 1.0
        for phi in (0.0, PHI):
            s.set_guidance_rescale(phi)
            lat = s.sample_latent(ctx, unc, 7.5, 5, init_latent=x_T)
            o64 = G.GuidanceOracle(synth, syn.alphas_cumprod(), d, torch.float64, "eps", phi)
            ref = _ref_txt2img(o64, ("default",), ctx, unc, 5, x_T).numpy()
            assert np.isfinite(lat).all()
            r[phi] = float(np.sqrt(np.mean((lat.astype(np.float64) - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
            max_f = max(max_f, o64.max_f)
            print(f"bf16 default sampler phi={phi}: rel-RMS vs fp64 = {r[phi]:.3e}  (largest f_b {o64.max_f:.4f})")
        assert r[0.0] < BAR_LATENT_BF16
        assert r[PHI] <= r[0.0] * max_f + BAR_LATENT_BF16, f"{r[PHI]:.3e} > {r[0.0]:.3e} x {max_f:.4f} + {BAR_LATENT_BF16}"
    finally:
        s.close()
