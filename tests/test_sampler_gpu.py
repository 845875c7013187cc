"""Sampler choice (include/sdmi.h "sampler choice") on the GPU through the C ABI: stochastic DDIM (eta), DPM-Solver++(2M) and
PLMS against the oracle driven by the TEXTBOOK forms of tests/sampler_ref.py (step noise from the numpy stream).  Bars as in test_model_gpu.py /
test_img2img_gpu.py: |gpu - f64| <= max(1e-3, 2 |f32 - f64|) on latents, <= 1 LSB on the u8 image."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import img2img_ref as R
import sampler_ref as S
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_STATE = -1, -6
BAR_LATENT_BF16 = 2.6e-2   # tests/test_bf16_gpu.py: 5-step CFG latent at precision 1
NOISE_SEED = 0x5EED
CASES = [("dpmpp_2m", 0.0), ("plms", 0.0), ("ddim", 0.5), ("ddim", 1.0)]


@pytest.fixture
def sd(sd_tiny):
    """the session's engine; whatever a test sets, the next test (of any file) finds the default sampler"""
    sd_tiny.set_sampler(None)
    yield sd_tiny
    sd_tiny.set_sampler(None)


def _new_sd(d, synth, precision=0, vae_encoder=True):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    s = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision))
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
    rng = np.random.default_rng(200 + seed)
    z0 = (rng.standard_normal((n, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    noise = np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, z0, noise


def _oracles(synth, d):
    a = syn.alphas_cumprod()
    return O.StableDiffusionOracle(synth, a, d, torch.float32), O.StableDiffusionOracle(synth, a, d, torch.float64)


def _half_mask(n, h, w):
    m = np.zeros((n, 1, h, w), np.float32)
    m[..., : w // 2 - 1] = 1.0
    m[..., w // 2 - 1] = 0.75
    m[..., w // 2] = 0.25
    return m


def _ref_txt2img(ora, ctx, unc, n_steps, x_T, kind, eta, image_base=0):
    ts, step = O.ddim_timesteps(n_steps, ora.n_steps)
    return S.sample_latent(ora, ctx, unc, 7.5, ts, step, x_T, kind, eta, NOISE_SEED, image_base)


def _ref_img2img(ora, ctx, unc, n_steps, strength, z0, eps, mask, kind, eta):
    ts, step = R.timesteps(n_steps, strength, ora.n_steps)
    a0 = float(ora.alphas[ts[0]])
    z0_, eps_ = torch.as_tensor(z0).to(ora.dtype), torch.as_tensor(eps).to(ora.dtype)
    x = math.sqrt(a0) * z0_ + math.sqrt(1.0 - a0) * eps_
    return S.sample_latent(ora, ctx, unc, 7.5, ts, step, x, kind, eta, NOISE_SEED, 0, mask, z0_ if mask is not None else None, eps_ if mask is not None else None)


# ---- 1. fp32 parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta", CASES)
def test_txt2img_parity(sd, synth, tiny_dims, kind, eta):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 2, 7, 3)
    o32, o64 = _oracles(synth, d)
    sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
    got = sd.sample_latent(ctx, unc, 7.5, 5, init_latent=x_T)
    img = sd.sample_image(ctx, unc, 7.5, 5, init_latent=x_T)
    assert np.array_equal(sd.latent_to_image(got), img), "image API != latent_to_image(latent API)"
    r32 = _ref_txt2img(o32, ctx, unc, 5, x_T, kind, eta).numpy()
    r64 = _ref_txt2img(o64, ctx, unc, 5, x_T, kind, eta)
    _assert_close(got, r32, r64.numpy(), f"txt2img {kind} eta={eta}")
    ref_img, _ = o64.latent_to_image(r64)
    di = int(np.abs(img.astype(np.int16) - ref_img.astype(np.int16)).max())
    print(f"txt2img {kind} eta={eta}: u8 max diff {di} LSB")
    assert di <= 1
    # and it is not the default sampler's result
    sd.set_sampler(None)
    assert not np.array_equal(sd.sample_latent(ctx, unc, 7.5, 5, init_latent=x_T), got)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,eta", CASES)
def test_img2img_latent_api_parity(sd, synth, tiny_dims, kind, eta, masked):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 5, 2, seed=1)
    mask = _half_mask(2, d.latent_h, d.latent_w) if masked else None
    o32, o64 = _oracles(synth, d)
    sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
    got = sd.sample_latent_from(ctx, unc, 7.5, 5, 0.6, z0, mask=mask, noise=noise)
    r32 = _ref_img2img(o32, ctx, unc, 5, 0.6, z0, noise, mask, kind, eta).numpy()
    r64 = _ref_img2img(o64, ctx, unc, 5, 0.6, z0, noise, mask, kind, eta).numpy()
    _assert_close(got, r32, r64, f"img2img {kind} eta={eta} masked={masked}")
    if masked:
        assert np.array_equal(got[..., -1], z0[..., -1])   # kept columns end exactly at z0 whatever the sampler


# ---- 2. nothing moved -----------------------------------------------------------------------------------------------------------------
def test_default_sampler_is_untouched(sd, synth, tiny_dims):
    """eta = 0 DDIM set explicitly, and the default restored after another sampler, against a context that never set one: same bits, same launches"""
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 7, 3, seed=2)
    mask = _half_mask(2, d.latent_h, d.latent_w)

    def calls(s):
        out = []
        for f in (lambda: s.sample_latent(ctx, unc, 7.5, 4, init_latent=noise),
                  lambda: s.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=mask, noise=noise),
                  lambda: s.sample_image(ctx, unc, 7.5, 4, init_latent=noise)):
            out.append((f(), s.last_call_stats()["kernels"]))
        return out

    fresh = _new_sd(d, synth)
    try:
        assert fresh.get_sampler() == {"kind": "ddim", "eta": 0.0, "noise_seed": 0, "image_base": 0}
        ref = calls(fresh)
    finally:
        fresh.close()
    sd.set_sampler("ddim", eta=0.0, noise_seed=77, image_base=5)
    assert sd.get_sampler() == {"kind": "ddim", "eta": 0.0, "noise_seed": 77, "image_base": 5}
    for (a, ka), (b, kb) in zip(calls(sd), ref):
        assert np.array_equal(a, b) and ka == kb
    sd.set_sampler("dpmpp_2m")
    assert sd.get_sampler()["kind"] == "dpmpp_2m"
    sd.set_sampler(None)
    assert sd.get_sampler() == {"kind": "ddim", "eta": 0.0, "noise_seed": 0, "image_base": 0}
    for (a, ka), (b, kb) in zip(calls(sd), ref):
        assert np.array_equal(a, b) and ka == kb


def test_invalid_samplers_are_refused_at_set_time(sd):
    from stable_diffusion_burn_amd._capi import SdmiSampler
    lib = sd._lib
    sd.set_sampler("ddim", eta=0.25, noise_seed=3, image_base=1)
    before = sd.get_sampler()
    for kind, eta in [(3, 0.0), (-1, 0.0), (0, -0.01), (0, 1.0001), (0, float("nan")), (1, 0.5), (2, 1.0)]:
        s = SdmiSampler()
        s.kind, s.eta = kind, eta
        assert lib.sdmi_set_sampler(sd._ctx, C.byref(s)) == SDMI_ERR_INVALID, (kind, eta)
        assert sd.get_sampler() == before   # nothing changes
    assert lib.sdmi_get_sampler(sd._ctx, None) == SDMI_ERR_INVALID


# ---- 3. one launch per step -------------------------------------------------------------------------------------------------------------
def test_one_update_launch_per_step(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 1, 7, 2, seed=3)
    mask = _half_mask(1, d.latent_h, d.latent_w)
    counts = {}
    for kind, eta in [("ddim", 0.0)] + CASES:
        sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
        sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise)
        a = sd.last_call_stats()["kernels"]
        sd.sample_latent_from(ctx, unc, 7.5, 5, 1.0, z0, mask=mask, noise=noise)
        counts[(kind, eta)] = (a, sd.last_call_stats()["kernels"])
    print(counts)
    assert len(set(counts.values())) == 1, counts


# ---- 4. partition independence --------------------------------------------------------------------------------------------------------
def test_batch_equals_single_calls_with_image_base(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 3, 7, 2, seed=4)
    sd.set_sampler("ddim", eta=1.0, noise_seed=NOISE_SEED)
    batch = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=x_T)
    wrong = None
    for i in range(3):
        sd.set_sampler("ddim", eta=1.0, noise_seed=NOISE_SEED, image_base=i)
        one = sd.sample_latent(ctx[i:i + 1], unc, 7.5, 4, init_latent=x_T[i:i + 1])
        scale = max(1.0, np.abs(one).max())
        err = np.abs(batch[i:i + 1] - one).max()
        print(f"image {i}: batch vs single max|d| = {err:.2e}")
        assert err <= 2e-5 * scale, f"image {i}"
        if i == 1:
            sd.set_sampler("ddim", eta=1.0, noise_seed=NOISE_SEED, image_base=0)
            wrong = sd.sample_latent(ctx[i:i + 1], unc, 7.5, 4, init_latent=x_T[i:i + 1])
    assert np.abs(batch[1:2] - wrong).max() > 1e-2   # the base matters: image 1 with image 0's noise is another image


def _multi_equals_single(sd, synth, d, devices):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=devices)
    try:
        m.load_weights(synth)
        n = 2 * len(devices) + 1
        lat = np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(n)])
        ctx = syn.cond_context(0, 7, d.ctx_dim)
        unc = syn.uncond_context(2, d.ctx_dim)
        for kind, eta in (("ddim", 1.0), ("dpmpp_2m", 0.0)):
            m.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
            sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
            got = m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat)
            ref = sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 3, init_latent=lat)
            for i in range(n):   # the bar of test_model_gpu.py::test_sharded_sample_image_through_the_c_abi
                assert np.array_equal(got[i], ref[i]), f"{kind}: image {i} of {n} on {len(devices)} device(s)"
        m.set_sampler(None)
        sd.set_sampler(None)
        assert np.array_equal(m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat), sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 3, init_latent=lat))
    finally:
        m.close()


def test_multi_context_with_one_device_equals_single(sd, synth, tiny_dims):
    _multi_equals_single(sd, synth, tiny_dims, (0,))


def test_multi_context_on_every_device_equals_single(sd, synth, tiny_dims):
    n_dev = torch.cuda.device_count()
    if n_dev < 2:
        pytest.skip("needs two or more devices")
    _multi_equals_single(sd, synth, tiny_dims, tuple(range(n_dev)))


# ---- 5. device-pointer variants -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,eta", [("dpmpp_2m", 0.0), ("plms", 0.0), ("ddim", 1.0)])
def test_dev_variants_equal_host_variants(sd, tiny_dims, kind, eta):
    d = tiny_dims
    n = 2
    ctx, unc, z0, noise = _inputs(d, n, 7, 3, seed=5)
    mask = _half_mask(n, d.latent_h, d.latent_w)
    sd.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
    host = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=noise)
    host_from = sd.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=mask, noise=noise)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(ctx=ctx, unc=unc, z0=z0, noise=noise, mask=mask).items()}
    lat = torch.empty((n, 4, d.latent_h, d.latent_w), dtype=torch.float32, device="cuda")
    sd.sample_latent_dev(t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, t["noise"].data_ptr(), lat.data_ptr())
    assert np.array_equal(lat.cpu().numpy(), host)
    sd.sample_latent_from_dev(t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["z0"].data_ptr(), t["mask"].data_ptr(),
                              t["noise"].data_ptr(), 0, lat.data_ptr())
    assert np.array_equal(lat.cpu().numpy(), host_from)


# ---- 6. history hygiene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dpmpp_2m", "plms"])
def test_no_history_leaks_across_calls(sd, tiny_dims, kind):
    d = tiny_dims
    ctx, unc, z0, noise = _inputs(d, 2, 7, 2, seed=6)
    sd.set_sampler(kind)
    a = sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise)
    other = sd.sample_latent(ctx, unc, 7.5, 3, init_latent=noise[::-1])   # leaves another history behind
    b = sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise)
    assert np.array_equal(a, b) and np.isfinite(other).all()
    # a failed call (bad strength) between two good ones
    lib = sd._lib
    F = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    out = np.empty_like(z0)
    good = sd.sample_latent_from(ctx, unc, 7.5, 5, 0.6, z0, noise=noise)
    for s in (0.0, 1.0001, float("nan"), 0.1):
        assert lib.sdmi_img2img_latent(sd._ctx, F(ctx), 2, 7, F(unc), 2, 7.5, 5, s, F(z0), None, F(noise), 0, F(out)) == SDMI_ERR_INVALID
    assert np.array_equal(sd.sample_latent_from(ctx, unc, 7.5, 5, 0.6, z0, noise=noise), good)
    assert np.array_equal(sd.sample_latent(ctx, unc, 7.5, 5, init_latent=noise), a)


def test_failed_calls_return_the_pool(tiny_dims, synth):
    """as test_img2img_gpu.py::test_no_encoder_weights, with a sampler that keeps history: failed calls return their pool blocks, the next good
    call's result is unchanged"""
    from stable_diffusion_burn_amd import SdmiError
    d = tiny_dims
    s = _new_sd(d, synth, vae_encoder=False)
    try:
        s.set_sampler("plms")
        ctx, unc, z0, noise = _inputs(d, 1, 7, 2)
        img = np.zeros((1, 8 * d.latent_h, 8 * d.latent_w, 3), np.uint8)
        ref = s.sample_latent_from(ctx, unc, 7.5, 4, 1.0, z0, noise=noise)
        assert np.isfinite(ref).all()
        for _ in range(20):
            with pytest.raises(SdmiError) as ei:
                s.sample_image_from(ctx, unc, 7.5, 4, 1.0, img, mask=np.ones((1, d.latent_h, d.latent_w), np.float32), noise=noise)
            assert ei.value.status == SDMI_ERR_STATE
        assert np.array_equal(s.sample_latent_from(ctx, unc, 7.5, 4, 1.0, z0, noise=noise), ref)
    finally:
        s.close()


# ---- 7. precision 1 -------------------------------------------------------------------------------------------------------------------
def test_precision_1(synth):
    """bf16: the rel-RMS of each sampler's 5-step latent against the fp64 restatement of the SAME sampler.  No bf16 figure exists for the new samplers, so
    the bar is relative to DDIM measured here on the unchanged path: r <= G r_ddim with G = the largest per-step 1-norm of the (normalised) weights the sampler
    puts on UNet outputs (sampler_ref.gain, from sdmi_sampler_coefs: 1 for DDIM, 1 + 1/r ~ 2 for DPM-Solver++(2M), 160/24 for PLMS) -- the worst-case gain
    of an extrapolation on its inputs' rounding error.  DDIM itself stays under BAR_LATENT_BF16.  DDIM at eta = 1 is printed with the others."""
    from stable_diffusion_burn_amd import sampler_coefs
    d = O.Dims(320, 8, 768, 8, 8, 64)   # bf16 needs channel counts that are multiples of 64 (tests/test_bf16_gpu.py)
    s = _new_sd(d, synth, precision=1, vae_encoder=False)
    try:
        ctx, unc, _, x_T = _inputs(d, 1, 77, 77, seed=7)
        o64 = O.StableDiffusionOracle(synth, syn.alphas_cumprod(), d, torch.float64)
        ts, step = O.ddim_timesteps(5, 1000)
        r, g = {}, {}
        for kind, eta in [("ddim", 0.0), ("dpmpp_2m", 0.0), ("plms", 0.0), ("ddim", 1.0)]:
            if (kind, eta) == ("ddim", 0.0):
                s.set_sampler(None)
            else:
                s.set_sampler(kind, eta=eta, noise_seed=NOISE_SEED)
            lat = s.sample_latent(ctx, unc, 7.5, 5, init_latent=x_T)
            ref = _ref_txt2img(o64, ctx, unc, 5, x_T, kind, eta).numpy()
            assert np.isfinite(lat).all()
            r[(kind, eta)] = float(np.sqrt(np.mean((lat.astype(np.float64) - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
            g[(kind, eta)] = S.gain(kind, sampler_coefs(kind, eta, syn.alphas_cumprod(), ts, step))
            print(f"bf16 {kind} eta={eta}: rel-RMS vs fp64 = {r[(kind, eta)]:.3e}  (G = {g[(kind, eta)]:.3f})")
        r_ddim = r[("ddim", 0.0)]
        assert r_ddim < BAR_LATENT_BF16
        assert g[("ddim", 0.0)] == 1.0 and 1.5 < g[("dpmpp_2m", 0.0)] < 3.0 and abs(g[("plms", 0.0)] - 160.0 / 24.0) < 1e-9
        for key in [("dpmpp_2m", 0.0), ("plms", 0.0)]:
            assert r[key] <= g[key] * r_ddim, f"{key}: {r[key]:.3e} > {g[key]:.3f} x {r_ddim:.3e}"
    finally:
        s.close()


# ---- 8. profile -----------------------------------------------------------------------------------------------------------------------
def test_sampler_step_profiles_as_other(sd, tiny_dims):
    d = tiny_dims
    ctx, unc, _, x_T = _inputs(d, 1, 7, 2)
    sd.sample_latent(ctx, unc, 7.5, 3, init_latent=x_T)
    try:
        sd.set_option("profile", 1)
        sd.set_option("profile_reset", 1)
        sd.sample_latent(ctx, unc, 7.5, 3, init_latent=x_T)
        base = sd.profile_stats()
        sd.set_sampler("plms")
        sd.set_option("profile_reset", 1)
        sd.sample_latent(ctx, unc, 7.5, 3, init_latent=x_T)
        got = sd.profile_stats()
    finally:
        sd.set_option("profile", 0)
    print({k: v for k, v in got.items() if k == "other"}, {k: v for k, v in base.items() if k == "other"})
    assert got["other"]["launches"] > 0 and got["other"]["ms"] > 0
    # the step kernel replaces the CFG + DDIM update one for one, in the same class: every class counts what it counted
    assert {k: v["launches"] for k, v in got.items()} == {k: v["launches"] for k, v in base.items()}
