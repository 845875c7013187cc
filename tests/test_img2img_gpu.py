"""img2img (include/sdmi.h "img2img") on the GPU through the C ABI, against the CPU restatement in
tests/img2img_ref.py (the oracle's encoder and sampler with rules 1-6).  Bars as in test_model_gpu.py:
|gpu - f64| <= max(1e-3, 2 |f32 - f64|) on latents, <= 1 LSB on the u8 image."""
import ctypes as C

import numpy as np
import pytest
import torch

import img2img_ref as R
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_STATE = -1, -6
BAR_LATENT_BF16 = 2.6e-2   # tests/test_bf16_gpu.py: 5-step CFG latent at precision 1


def _assert_close(got, ref32, ref64, what, atol=1e-3):
    got, r32, r64 = (np.asarray(a, np.float64) for a in (got, ref32, ref64))
    assert np.isfinite(got).all(), f"{what}: non-finite"
    e64, e32 = np.abs(got - r64).max(), np.abs(r32 - r64).max()
    bound = max(atol, 2 * e32)
    assert e64 <= bound, f"{what}: max|gpu-f64|={e64:.3e} > {bound:.3e} (|f32-f64|={e32:.3e})"
    return e64, e32


def _inputs(d, n, T, Tu, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(Tu, d.ctx_dim)
    rng = np.random.default_rng(100 + seed)
    img = rng.integers(0, 256, (n, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=np.uint8)
    z0 = (rng.standard_normal((n, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    noise = np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(n)])
    return ctx, unc, img, z0, noise


def _oracles(synth, d):
    a = syn.alphas_cumprod()
    return O.StableDiffusionOracle(synth, a, d, torch.float32), O.StableDiffusionOracle(synth, a, d, torch.float64)


def _half_mask(n, h, w):
    """left half regenerates, right half is kept, a soft band of two columns in between"""
    m = np.zeros((n, 1, h, w), np.float32)
    m[..., : w // 2 - 1] = 1.0
    m[..., w // 2 - 1] = 0.75
    m[..., w // 2] = 0.25
    return m


@pytest.mark.parametrize("strength", [0.3, 0.75, 1.0])
def test_image_api_parity(sd_tiny, synth, tiny_dims, strength):
    d = tiny_dims
    ctx, unc, img, _, noise = _inputs(d, 2, 7, 3)
    o32, o64 = _oracles(synth, d)
    got = sd_tiny.sample_image_from(ctx, unc, 7.5, 4, strength, img, noise=noise)
    # the image API's latent: the latent API started from the GPU encoder's z0 (same fp32 input, same kernels) is the same call
    x = R.rgb_to_model_input(img)
    z0_gpu = sd_tiny.autoencoder.encode_image(x) * R.VAE_SCALE
    lat = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, strength, z0_gpu, noise=noise)
    assert np.array_equal(sd_tiny.latent_to_image(lat), got), "image API != latent_to_image(latent API(0.18215 encode(x)))"
    refs = []
    for o in (o32, o64):
        z0 = R.encode_z0(O.EncoderOracle(synth, d, o.dtype), img)
        refs.append(R.sample_latent_from(o, ctx, unc, 7.5, 4, strength, z0, noise))
    e64, e32 = _assert_close(lat, refs[0].numpy(), refs[1].numpy(), f"img2img latent strength={strength}")
    ref_img, _ = o64.latent_to_image(refs[1])
    di = int(np.abs(got.astype(np.int16) - ref_img.astype(np.int16)).max())
    print(f"img2img strength={strength}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}; u8 max diff {di} LSB")
    assert di <= 1


def test_latent_api_masked_parity(sd_tiny, synth, tiny_dims):
    d = tiny_dims
    ctx, unc, _, z0, noise = _inputs(d, 2, 5, 2, seed=1)
    mask = _half_mask(2, d.latent_h, d.latent_w)
    o32, o64 = _oracles(synth, d)
    got = sd_tiny.sample_latent_from(ctx, unc, 7.5, 5, 0.6, z0, mask=mask, noise=noise)
    r32 = R.sample_latent_from(o32, ctx, unc, 7.5, 5, 0.6, z0, noise, mask).numpy()
    r64 = R.sample_latent_from(o64, ctx, unc, 7.5, 5, 0.6, z0, noise, mask).numpy()
    e64, e32 = _assert_close(got, r32, r64, "img2img masked latent")
    print(f"img2img masked: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    assert np.array_equal(got[..., -1], z0[..., -1])   # kept columns end exactly at z0
    # pixel-resolution mask of the image API: the 8x8 max -> the same latent mask
    _, _, img, _, _ = _inputs(d, 1, 5, 2, seed=1)
    pm = np.zeros((1, 8 * d.latent_h, 8 * d.latent_w), bool)
    pm[:, :, : 8 * (d.latent_w // 2) - 3] = True   # touches latent column w/2 - 1
    lm = np.zeros((1, d.latent_h, d.latent_w), np.float32)
    lm[:, :, : d.latent_w // 2] = 1.0
    a = sd_tiny.sample_image_from(ctx[:1], unc, 7.5, 5, 0.6, img, mask=pm, noise=noise[:1])
    b = sd_tiny.sample_image_from(ctx[:1], unc, 7.5, 5, 0.6, img, mask=lm, noise=noise[:1])
    assert np.array_equal(a, b)


def test_full_strength_zero_z0_is_txt2img(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, _, _, noise = _inputs(d, 2, 7, 2)
    z0 = np.zeros_like(noise)
    got = sd_tiny.sample_latent_from(ctx, unc, 7.5, 3, 1.0, z0, noise=noise)
    ks = sd_tiny.last_call_stats()["kernels"]
    s = np.float32(np.sqrt(1.0 - np.float64(syn.alphas_cumprod()[999])))
    ref = sd_tiny.sample_latent(ctx, unc, 7.5, 3, init_latent=s * noise)
    assert np.array_equal(got, ref)
    assert ks == sd_tiny.last_call_stats()["kernels"] - 1   # one start kernel instead of the layout conversion + dup_latent


def test_mask_of_ones_and_zeros(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, _, z0, noise = _inputs(d, 2, 7, 2, seed=2)
    plain = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, noise=noise)
    ones = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=np.ones((2, d.latent_h, d.latent_w), np.float32), noise=noise)
    assert np.array_equal(plain, ones)
    zeros = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=np.zeros((2, 1, d.latent_h, d.latent_w), np.float32), noise=noise)
    assert np.array_equal(zeros, z0)
    again = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, noise=noise)
    assert np.array_equal(plain, again)


def test_dev_variants_equal_host_variants(sd_tiny, tiny_dims):
    d = tiny_dims
    n = 2
    ctx, unc, img, z0, noise = _inputs(d, n, 7, 3, seed=3)
    mask = _half_mask(n, d.latent_h, d.latent_w)
    host_lat = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=mask, noise=noise)
    host_img = sd_tiny.sample_image_from(ctx, unc, 7.5, 4, 0.75, img, mask=mask, noise=noise)
    host_seed = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, seed=9)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(ctx=ctx, unc=unc, img=img, z0=z0, noise=noise, mask=mask).items()}
    lat = torch.empty((n, 4, d.latent_h, d.latent_w), dtype=torch.float32, device="cuda")
    rgb = torch.empty((n, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=torch.uint8, device="cuda")
    sd_tiny.sample_latent_from_dev(t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["z0"].data_ptr(), t["mask"].data_ptr(),
                                   t["noise"].data_ptr(), 0, lat.data_ptr())
    assert np.array_equal(lat.cpu().numpy(), host_lat)
    sd_tiny.sample_image_from_dev(t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["img"].data_ptr(), t["mask"].data_ptr(),
                                  t["noise"].data_ptr(), 0, rgb.data_ptr())
    assert np.array_equal(rgb.cpu().numpy(), host_img)
    sd_tiny.sample_latent_from_dev(t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["z0"].data_ptr(), None, None, 9,
                                   lat.data_ptr())
    assert np.array_equal(lat.cpu().numpy(), host_seed)


def test_seed_path_matches_the_numpy_stream(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, _, z0, _ = _inputs(d, 3, 7, 2, seed=4)
    seeded = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, seed=41)
    explicit = sd_tiny.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, noise=R.seeded_noise(41, 3, d.latent_h, d.latent_w))
    err = np.abs(seeded - explicit).max()
    print(f"seeded vs numpy stream: max|d| = {err:.2e}")
    assert err <= 1e-3 * max(1.0, np.abs(explicit).max())
    # the txt2img seed path draws the same eps: sample_latent(seed) starts from eps, img2img at strength 1 with z0 = 0 from sqrt(1 - a_999) eps
    for i in range(3):
        one = sd_tiny.sample_latent_from(ctx[i:i + 1], unc, 7.5, 4, 0.75, z0[i:i + 1], seed=41 + i)
        scale = max(1.0, np.abs(one).max())
        assert np.abs(seeded[i:i + 1] - one).max() <= 2e-5 * scale, f"image {i}"


def test_image_api_seed_path(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, img, _, _ = _inputs(d, 2, 7, 2, seed=5)
    seeded = sd_tiny.sample_image_from(ctx, unc, 7.5, 4, 0.5, img, seed=7)
    explicit = sd_tiny.sample_image_from(ctx, unc, 7.5, 4, 0.5, img, noise=R.seeded_noise(7, 2, d.latent_h, d.latent_w))
    assert int(np.abs(seeded.astype(np.int16) - explicit.astype(np.int16)).max()) <= 1


def test_precision_1(synth):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    d = O.Dims(320, 8, 768, 8, 8, 64)   # bf16 needs channel counts that are multiples of 64 (tests/test_bf16_gpu.py)
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=1))
    try:
        sd.load_weights(synth, clip=False)
        ctx, unc, img, _, noise = _inputs(d, 1, 77, 77, seed=6)
        o64 = O.StableDiffusionOracle(synth, syn.alphas_cumprod(), d, torch.float64)
        z0 = R.encode_z0(O.EncoderOracle(synth, d, torch.float64), img)
        ref = R.sample_latent_from(o64, ctx, unc, 7.5, 5, 0.6, z0, noise).numpy()
        got_img = sd.sample_image_from(ctx, unc, 7.5, 5, 0.6, img, noise=noise)
        lat = sd.sample_latent_from(ctx, unc, 7.5, 5, 0.6, sd.autoencoder.encode_image(R.rgb_to_model_input(img)) * R.VAE_SCALE, noise=noise)
        assert np.array_equal(sd.latent_to_image(lat), got_img)
        r = float(np.sqrt(np.mean((lat.astype(np.float64) - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))
        print(f"bf16 img2img latent: rel-RMS vs fp64 = {r:.3e}")
        assert np.isfinite(lat).all() and r < BAR_LATENT_BF16
    finally:
        sd.close()


def test_bad_strength_is_invalid(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, img, z0, _ = _inputs(d, 1, 7, 2)
    lib = sd_tiny._lib
    F = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    out = np.empty_like(z0)
    rgb = np.empty_like(img)
    for s in (0.0, -0.1, 1.0001, float("nan"), 0.1):   # 0.1 * 4 steps < 1
        assert lib.sdmi_img2img_latent(sd_tiny._ctx, F(ctx), 1, 7, F(unc), 2, 7.5, 4, s, F(z0), None, None, 0, F(out)) == SDMI_ERR_INVALID
        assert lib.sdmi_img2img_image(sd_tiny._ctx, F(ctx), 1, 7, F(unc), 2, 7.5, 4, s, img.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, 0,
                                      rgb.ctypes.data_as(C.POINTER(C.c_uint8))) == SDMI_ERR_INVALID


def test_no_encoder_weights(tiny_dims, synth):
    """the image API needs the encoder group (SDMI_ERR_STATE, as sdmi_encode_image); the latent API does not.  Failed calls
    return their pool blocks: the next good call's result is unchanged."""
    from stable_diffusion_burn_amd import ModelConfig, SdmiError, StableDiffusion
    d = tiny_dims
    sd = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch))
    try:
        sd.load_weights(synth, clip=False, vae_encoder=False)
        ctx, unc, img, z0, noise = _inputs(d, 1, 7, 2)
        ref = sd.sample_latent_from(ctx, unc, 7.5, 2, 1.0, z0, noise=noise)
        assert np.isfinite(ref).all()
        for _ in range(20):
            with pytest.raises(SdmiError) as ei:
                sd.sample_image_from(ctx, unc, 7.5, 2, 1.0, img, mask=np.ones((1, d.latent_h, d.latent_w), np.float32), noise=noise)
            assert ei.value.status == SDMI_ERR_STATE
        assert np.array_equal(sd.sample_latent_from(ctx, unc, 7.5, 2, 1.0, z0, noise=noise), ref)
    finally:
        sd.close()


def test_new_kernels_profile_as_other(sd_tiny, tiny_dims):
    d = tiny_dims
    ctx, unc, img, _, _ = _inputs(d, 1, 7, 2)
    mask = _half_mask(1, d.latent_h, d.latent_w)
    sd_tiny.sample_image(ctx, unc, 7.5, 2, init_latent=syn.initial_latent(0, d.latent_h, d.latent_w)[None])
    try:
        sd_tiny.set_option("profile", 1)
        sd_tiny.set_option("profile_reset", 1)
        sd_tiny.sample_image(ctx, unc, 7.5, 2, init_latent=syn.initial_latent(0, d.latent_h, d.latent_w)[None])
        base = sd_tiny.profile_stats()
        sd_tiny.set_option("profile_reset", 1)
        sd_tiny.sample_image_from(ctx, unc, 7.5, 2, 1.0, img, mask=mask, seed=3)
        got = sd_tiny.profile_stats()
    finally:
        sd_tiny.set_option("profile", 0)
    print({k: v for k, v in got.items() if k == "other"}, {k: v for k, v in base.items() if k == "other"})
    assert got["other"]["launches"] > 0 and got["other"]["ms"] > 0
