"""Per-call latent size and the hires fix (include/sdmi.h "latent size per call" / "hires fix") on the GPU through the C ABI:
the resampler against the float64 tables (tests/resize_ref.py), the size setter against a fresh context, the hires call against the oracle's pieces
and against the composition of the public calls it fuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import img2img_ref as R
import resize_ref as RR
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

pytestmark = pytest.mark.gpu

SDMI_ERR_INVALID, SDMI_ERR_STATE = -1, -6
U = 2.0 ** -24
BASE, FINAL = (8, 8), (16, 16)
BF16_DIMS = O.Dims(320, 8, 768, 16, 16, 64)   # bf16 needs channel counts that are multiples of 64 (tests/test_bf16_gpu.py)


def _new_sd(d, synth, h, w, precision=0, vae_encoder=False):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    s = StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, h, w, d.vae_ch, precision=precision))
    s.load_weights(synth, clip=False, vae_encoder=vae_encoder)
    return s


@pytest.fixture
def sd(sd_tiny, tiny_dims):
    """the session's engine (created at 16 x 16); whatever a test sets, the next test (of any file) finds that size and the default sampler"""
    sd_tiny.set_sampler(None)
    sd_tiny.set_latent_size(tiny_dims.latent_h, tiny_dims.latent_w)
    yield sd_tiny
    sd_tiny.set_sampler(None)
    sd_tiny.set_latent_size(tiny_dims.latent_h, tiny_dims.latent_w)


def _prompts(d, n, T=7, Tu=3):
    return np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)]), syn.uncond_context(Tu, d.ctx_dim)


def _latents(n, h, w, first=0):
    return np.stack([syn.initial_latent(first + i, h, w) for i in range(n)])


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------------
def _check_resize(sd_ops, h, w, oh, ow, mode, aa, n=2):
    x = np.random.default_rng(h * 1000 + w * 10 + mode).standard_normal((n, 4, h, w)).astype(np.float32)
    got = sd_ops.op_resize(x, (oh, ow), RR.MODES[mode], bool(aa))
    ref, s, tx, ty = RR.resize(x, oh, ow, mode, aa)
    assert got.shape == ref.shape and np.isfinite(got).all()
    if mode == 0:
        assert np.array_equal(got, ref.astype(np.float32)), "nearest is a gather"
        return
    # two fp32 dot products of T terms (with or without fma), one fp32 rounding of each weight per axis and of the intermediate
    bound = (tx + ty + 8) * U * s
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{h}x{w} -> {oh}x{ow} mode {mode} aa {aa}: taps {ty} x {tx}, max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("h,w,oh,ow", [(16, 16, 24, 32), (8, 8, 16, 16), (8, 24, 20, 8)])
def test_resize_kernel(sd_ops, h, w, oh, ow, mode):
    _check_resize(sd_ops, h, w, oh, ow, mode, 0)


@pytest.mark.parametrize("mode", [1, 2])
def test_resize_kernel_antialiased(sd_ops, mode):
    _check_resize(sd_ops, 24, 16, 8, 8, mode, 1)


@pytest.mark.parametrize("mode", [0, 1])
def test_resize_kernel_past_one_grid(sd_ops, mode):
    """more output pixels than the launch has threads (2048 workgroups x 256): the grid-stride loop's second trip"""
    assert 736 * 720 > 2048 * 256
    _check_resize(sd_ops, 16, 16, 736, 720, mode, 0, n=1)


@pytest.mark.parametrize("mode,aa", [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1)])
def test_resize_identity_returns_its_input(sd_ops, mode, aa):
    x = np.random.default_rng(5).standard_normal((2, 4, 8, 24)).astype(np.float32)
    x[0, 0, 0, 0] = -0.0
    got = sd_ops.op_resize(x, (8, 24), RR.MODES[mode], bool(aa))
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_resize_is_deterministic_skips_identity_axes_and_profiles_as_other(sd_ops):
    x = np.random.default_rng(6).standard_normal((2, 4, 8, 24)).astype(np.float32)
    a = sd_ops.op_resize(x, (20, 8), "bicubic")
    k_both = sd_ops.last_call_stats()["kernels"]
    assert np.array_equal(sd_ops.op_resize(x, (20, 8), "bicubic"), a)
    sd_ops.op_resize(x, (8, 8), "bicubic")
    k_w = sd_ops.last_call_stats()["kernels"]
    sd_ops.op_resize(x, (20, 24), "bicubic")
    k_h = sd_ops.last_call_stats()["kernels"]
    assert (k_both, k_w, k_h) == (4, 3, 3)     # two layout converters + one launch per axis that changes
    try:
        sd_ops.set_option("profile", 1)
        sd_ops.set_option("profile_reset", 1)
        sd_ops.op_resize(x, (20, 8), "bicubic")
        st = sd_ops.profile_stats()
    finally:
        sd_ops.set_option("profile", 0)
    assert st["other"]["launches"] == 4 and sum(v["launches"] for v in st.values()) == 4


def test_resize_argument_errors(sd_ops):
    from stable_diffusion_burn_amd import SdmiError
    x = np.zeros((1, 4, 8, 8), np.float32)
    for mode, aa in [(3, False), (-1, False), (0, True)]:
        with pytest.raises(SdmiError) as ei:
            sd_ops.op_resize(x, (16, 16), mode, aa)
        assert ei.value.status == SDMI_ERR_INVALID


# ---- 2. the size setter -------------------------------------------------------------------------------------------------------------------
def _size_calls(s, d, h, w):
    """every entry point that reads the size, at h x w"""
    ctx, unc = _prompts(d, 2)
    x_T, z0 = _latents(2, h, w), 0.8 * _latents(2, h, w, first=20)
    noise = _latents(2, h, w, first=40)
    lat = s.sample_latent(ctx, unc, 7.5, 3, init_latent=x_T)
    return {
        "sample_latent": lat,
        "sample_latent seeded": s.sample_latent(ctx, unc, 7.5, 2, seed=11),
        "sample_image": s.sample_image(ctx, unc, 7.5, 3, init_latent=x_T),
        "unet.forward": s.unet.forward(x_T, 500, ctx),
        "sample_latent_from": s.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=noise),
        "latent_to_image": s.latent_to_image(lat),
        "decode_latent": s.autoencoder.decode_latent(lat[:1]),
    }


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k


def test_set_latent_size_equals_a_fresh_context(sd, synth, tiny_dims):
    d = tiny_dims
    assert sd.latent_size == (16, 16)
    own = _size_calls(sd, d, 16, 16)
    sd.set_latent_size(8, 24)
    assert sd.latent_size == (8, 24) and (sd.config.latent_h, sd.config.latent_w) == (16, 16)
    got = _size_calls(sd, d, 8, 24)
    assert got["sample_latent"].shape == (2, 4, 8, 24) and got["sample_image"].shape == (2, 64, 192, 3)
    fresh = _new_sd(d, synth, 8, 24)
    try:
        _same(got, _size_calls(fresh, d, 8, 24))
    finally:
        fresh.close()
    sd.set_latent_size(16, 16)
    _same(_size_calls(sd, d, 16, 16), own)
    # refused sizes change nothing
    for h, w in [(12, 16), (16, 12), (0, 16), (16, 0), (-8, 16), (16, -8), (7, 7)]:
        assert sd._lib.sdmi_set_latent_size(sd._ctx, h, w) == SDMI_ERR_INVALID, (h, w)
        assert sd.latent_size == (16, 16)
    assert sd._lib.sdmi_get_latent_size(sd._ctx, None, None) == SDMI_ERR_INVALID
    _same(_size_calls(sd, d, 16, 16), own)
    # the Python shape checks follow the current size
    with pytest.raises(ValueError):
        sd.sample_latent(*_prompts(d, 2), 7.5, 3, init_latent=_latents(2, 8, 24))


def test_set_latent_size_with_the_encoder(sd, synth, tiny_dims):
    """encode_image and the image form of img2img read the current size too"""
    d = tiny_dims
    ctx, unc = _prompts(d, 1)
    img = np.random.default_rng(3).integers(0, 256, (1, 64, 192, 3), dtype=np.uint8)
    x = R.rgb_to_model_input(img)
    noise = _latents(1, 8, 24, first=40)
    sd.set_latent_size(8, 24)
    got = (sd.autoencoder.encode_image(x), sd.sample_image_from(ctx, unc, 7.5, 4, 0.5, img, noise=noise))
    fresh = _new_sd(d, synth, 8, 24, vae_encoder=True)
    try:
        ref = (fresh.autoencoder.encode_image(x), fresh.sample_image_from(ctx, unc, 7.5, 4, 0.5, img, noise=noise))
    finally:
        fresh.close()
    assert got[0].shape == (1, 4, 8, 24) and np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.fixture(scope="module")
def sd_bf16(synth):
    s = _new_sd(BF16_DIMS, synth, 16, 16, precision=1)
    yield s
    s.close()


def test_set_latent_size_precision_1(sd_bf16, synth):
    d = BF16_DIMS
    ctx, unc = _prompts(d, 2)
    x_T = _latents(2, 8, 24)
    own = sd_bf16.sample_latent(ctx, unc, 7.5, 2, init_latent=_latents(2, 16, 16))
    sd_bf16.set_latent_size(8, 24)
    try:
        got = sd_bf16.sample_latent(ctx, unc, 7.5, 2, init_latent=x_T)
    finally:
        sd_bf16.set_latent_size(16, 16)
    fresh = _new_sd(d, synth, 8, 24, precision=1)
    try:
        assert np.array_equal(got, fresh.sample_latent(ctx, unc, 7.5, 2, init_latent=x_T))
    finally:
        fresh.close()
    assert np.array_equal(sd_bf16.sample_latent(ctx, unc, 7.5, 2, init_latent=_latents(2, 16, 16)), own)


def _multi(d, devices):
    from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion
    return MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch), devices=devices)


def test_multi_context_follows_set_latent_size(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd import SdmiError
    d = tiny_dims
    m = _multi(d, (0,))
    try:
        m.load_weights(synth)
        m.set_latent_size(8, 24)
        assert m.latent_size == (8, 24)
        sd.set_latent_size(8, 24)
        n = 3
        lat = _latents(n, 8, 24)
        ctx, unc = syn.cond_context(0, 7, d.ctx_dim), syn.uncond_context(2, d.ctx_dim)
        got = m.sample_image(ctx, unc, 7.5, 3, n, init_latents=lat)
        ref = sd.sample_image(np.repeat(ctx[None], n, axis=0), unc, 7.5, 3, init_latent=lat)
        assert got.shape == (n, 64, 192, 3) and np.array_equal(got, ref)
        with pytest.raises(SdmiError) as ei:
            m.set_latent_size(8, 12)
        assert ei.value.status == SDMI_ERR_INVALID
        assert m.latent_size == (8, 24)
    finally:
        m.close()


def test_sharded_call_refuses_contexts_of_different_sizes(synth, tiny_dims):
    from stable_diffusion_burn_amd import SdmiError
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two or more devices")
    d = tiny_dims
    m = _multi(d, (0, 1))
    try:
        m.load_weights(synth)
        m.device_view(1).set_latent_size(8, 24)
        with pytest.raises(SdmiError) as ei:
            m.sample_image(syn.cond_context(0, 7, d.ctx_dim), syn.uncond_context(2, d.ctx_dim), 7.5, 2, 2, init_latents=_latents(2, 16, 16))
        assert ei.value.status == SDMI_ERR_STATE
    finally:
        m.close()


# ---- 3. hires against the oracle ----------------------------------------------------------------------------------------------------------
HIRES_STEPS, HIRES_STRENGTH = 4, 0.5     # int(0.5 * 4) = 2 steps in the second pass after 3 in the first: 5 in all, as the plain call


def _hires_inputs(d):
    ctx, unc = _prompts(d, 1, 7, 3)
    return ctx, unc, _latents(1, *BASE), _latents(1, *FINAL, first=30), _latents(1, *FINAL, first=60)


def _oracle_figures(ora, d):
    """in the oracle's dtype: the plain 5-step latent at the final size, the 3-step latent at the base size, and per mode the composed hires reference"""
    ctx, unc, x_base, x_final, hires_noise = _hires_inputs(d)
    t = torch.from_numpy
    plain = ora.sample_latent(t(ctx), t(unc), 7.5, 5, t(x_final)).numpy()
    base = ora.sample_latent(t(ctx), t(unc), 7.5, 3, t(x_base)).numpy()
    hires = {}
    for mode in (1, 2):
        z0, _, _, _ = RR.resize(base, *FINAL, mode, 0)
        hires[mode] = R.sample_latent_from(ora, ctx, unc, 7.5, HIRES_STEPS, HIRES_STRENGTH, z0, hires_noise).numpy()
    return plain, hires


def _hires_vs_plain(s, d, refs, what):
    ctx, unc, x_base, x_final, hires_noise = _hires_inputs(d)
    plain_ref, hires_ref = refs
    assert len(R.timesteps(HIRES_STEPS, HIRES_STRENGTH)[0]) == 2
    plain = _rel_rms(s.sample_latent(ctx, unc, 7.5, 5, init_latent=x_final), plain_ref)
    out = {}
    for mode in (1, 2):
        got = s.sample_latent_hires(ctx, unc, 7.5, 3, BASE, HIRES_STRENGTH, mode=RR.MODES[mode], hires_steps=HIRES_STEPS, init_latent=x_base,
                                    hires_noise=hires_noise)
        assert got.shape == (1, 4, *FINAL) and np.isfinite(got).all()
        out[mode] = _rel_rms(got, hires_ref[mode])
        print(f"{what} {RR.MODES[mode]}: rel-RMS hires = {out[mode]:.3e}, plain 5-step = {plain:.3e}")
    for mode in (1, 2):
        # equal step counts; the chain adds the resample (test 1: far below either figure) and one re-noise: a factor of 2 is the room for another
        # trajectory through the same nonlinear network
        assert out[mode] <= 2 * plain, f"{what} {RR.MODES[mode]}: {out[mode]:.3e} > 2 x {plain:.3e}"


@pytest.fixture(scope="module")
def oracle_refs_fp32(synth, tiny_dims):
    return _oracle_figures(O.StableDiffusionOracle(synth, syn.alphas_cumprod(), tiny_dims, torch.float64), tiny_dims)


def test_hires_against_the_oracle(sd, tiny_dims, oracle_refs_fp32):
    """rel-RMS of the hires latent against the composed float64 reference <= 2 x that of a plain 5-step sample_latent; both are printed.
    Measured on an MI355X: bilinear 1.273e-06, bicubic 1.372e-06, plain 1.374e-06; precision 1: 1.558e-02, 1.660e-02, 1.471e-02."""
    _hires_vs_plain(sd, tiny_dims, oracle_refs_fp32, "fp32")


def test_hires_against_the_oracle_precision_1(sd_bf16, synth):
    """bf16: the two figures, and hires <= 2 x plain with the plain figure measured here at precision 1.  The reference is the float32 oracle: its own
    error (about 1e-5 relative at these depths, tests/test_model_gpu.py) is three orders below either bf16 figure, at a third of the float64 oracle's time."""
    d = BF16_DIMS
    refs = _oracle_figures(O.StableDiffusionOracle(synth, syn.alphas_cumprod(), d, torch.float32), d)
    _hires_vs_plain(sd_bf16, d, refs, "bf16")


# ---- 4. fused equals composed ---------------------------------------------------------------------------------------------------------------
def _composed(s, ctx, unc, n_steps, x_base, mode, aa, hires_steps, strength, hires_noise):
    final = s.latent_size
    try:
        s.set_latent_size(*BASE)
        base = s.sample_latent(ctx, unc, 7.5, n_steps, init_latent=x_base)
    finally:
        s.set_latent_size(*final)
    z0 = s.op_resize(base, final, RR.MODES[mode], bool(aa))
    return s.sample_latent_from(ctx, unc, 7.5, hires_steps, strength, z0, noise=hires_noise)


@pytest.mark.parametrize("mode,aa,sampler", [(0, 0, None), (1, 0, None), (2, 0, None), (2, 1, None), (2, 0, "dpmpp_2m")])
def test_hires_equals_the_composition_of_public_calls(sd, tiny_dims, mode, aa, sampler):
    d = tiny_dims
    n = 2
    ctx, unc = _prompts(d, n)
    x_base, hires_noise = _latents(n, *BASE), _latents(n, *FINAL, first=60)
    if sampler:
        sd.set_sampler(sampler)
    ref = _composed(sd, ctx, unc, 3, x_base, mode, aa, HIRES_STEPS, 0.75, hires_noise)
    got = sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.75, mode=RR.MODES[mode], antialias=bool(aa), hires_steps=HIRES_STEPS, init_latent=x_base,
                                 hires_noise=hires_noise)
    assert np.array_equal(got, ref)
    img = sd.sample_image_hires(ctx, unc, 7.5, 3, BASE, 0.75, mode=RR.MODES[mode], antialias=bool(aa), hires_steps=HIRES_STEPS, init_latent=x_base,
                                hires_noise=hires_noise)
    assert img.shape == (n, 128, 128, 3) and np.array_equal(img, sd.latent_to_image(ref))
    assert sd.latent_size == FINAL


def _close_to_numpy_stream(got, explicit, what):
    """the bar of test_img2img_gpu.py::test_seed_path_matches_the_numpy_stream: tests/img2img_ref.py restates the device's N(0,1) stream with numpy's
    log / cos, which differ from the device's in the last bits, so a seeded call and the call given that restatement agree to 1e-3, not bit for bit"""
    err = np.abs(got - explicit).max()
    print(f"{what}: seeded vs numpy stream max|d| = {err:.2e}")
    assert err <= 1e-3 * max(1.0, np.abs(explicit).max())


def test_hires_defaults_and_seeds(sd, tiny_dims):
    """hires_steps 0 = n_steps; hires_noise None = image i's stream hires_seed + i; init_latent None = image i's stream seed + i at the base size --
    bit for bit the draws of the public calls' own seed paths, and the numpy restatement of the stream within its bar; base == final is sample_latent
    followed by its img2img tail, the resize being the identity"""
    d = tiny_dims
    n = 2
    ctx, unc = _prompts(d, n)
    x_base = _latents(n, *BASE)
    seeded = R.seeded_noise(77, n, *FINAL).astype(np.float32)
    a = sd.sample_latent_hires(ctx, unc, 7.5, 4, BASE, 0.5, mode="bilinear", init_latent=x_base, hires_seed=77)
    assert np.array_equal(a, sd.sample_latent_hires(ctx, unc, 7.5, 4, BASE, 0.5, mode="bilinear", hires_steps=4, init_latent=x_base, hires_seed=77))
    sd.set_latent_size(*BASE)
    base = sd.sample_latent(ctx, unc, 7.5, 4, init_latent=x_base)
    base_seeded = sd.sample_latent(ctx, unc, 7.5, 3, seed=5)
    sd.set_latent_size(*FINAL)
    assert np.array_equal(a, sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, sd.op_resize(base, FINAL, "bilinear"), seed=77))
    _close_to_numpy_stream(a, sd.sample_latent_hires(ctx, unc, 7.5, 4, BASE, 0.5, mode="bilinear", init_latent=x_base, hires_noise=seeded), "hires_seed")
    b = sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.5, mode="bilinear", hires_steps=4, seed=5, hires_noise=seeded)
    assert np.array_equal(b, sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, sd.op_resize(base_seeded, FINAL, "bilinear"), noise=seeded))
    x_seed = R.seeded_noise(5, n, *BASE).astype(np.float32)
    _close_to_numpy_stream(b, sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.5, mode="bilinear", hires_steps=4, init_latent=x_seed, hires_noise=seeded), "seed")
    x_T = _latents(n, *FINAL)
    same = sd.sample_latent_hires(ctx, unc, 7.5, 3, FINAL, 0.5, mode="bicubic", hires_steps=4, init_latent=x_T, hires_noise=seeded)
    assert np.array_equal(same, sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, sd.sample_latent(ctx, unc, 7.5, 3, init_latent=x_T), noise=seeded))


def test_hires_dev_forms_equal_host_forms(sd, tiny_dims):
    d = tiny_dims
    n = 2
    ctx, unc = _prompts(d, n)
    x_base, hires_noise = _latents(n, *BASE), _latents(n, *FINAL, first=60)
    sd.set_sampler("dpmpp_2m")
    host = sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.75, mode="bicubic", hires_steps=HIRES_STEPS, init_latent=x_base, hires_noise=hires_noise)
    host_seeded = sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.75, mode="bicubic", hires_steps=HIRES_STEPS, init_latent=x_base, hires_seed=9)
    host_img = sd.latent_to_image(host)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(ctx=ctx, unc=unc, x=x_base, noise=hires_noise).items()}
    lat = torch.empty((n, 4, *FINAL), dtype=torch.float32, device="cuda")
    rgb = torch.empty((n, 128, 128, 3), dtype=torch.uint8, device="cuda")
    args = (t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 3, BASE, 0.75, t["x"].data_ptr())
    sd.sample_latent_hires_dev(*args, t["noise"].data_ptr(), lat.data_ptr(), mode="bicubic", hires_steps=HIRES_STEPS)
    assert np.array_equal(lat.cpu().numpy(), host)
    sd.sample_latent_hires_dev(*args, None, lat.data_ptr(), mode="bicubic", hires_steps=HIRES_STEPS, hires_seed=9)
    assert np.array_equal(lat.cpu().numpy(), host_seeded)
    sd.sample_image_hires_dev(*args, t["noise"].data_ptr(), rgb.data_ptr(), mode="bicubic", hires_steps=HIRES_STEPS)
    assert np.array_equal(rgb.cpu().numpy(), host_img)


# ---- 5. nothing else moved ------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moved(sd, synth, tiny_dims):
    from stable_diffusion_burn_amd._capi import SdmiHires
    d = tiny_dims
    n = 2
    ctx, unc = _prompts(d, n)
    x_T, x_base = _latents(n, *FINAL), _latents(n, *BASE)

    def plain(s):
        lat = s.sample_latent(ctx, unc, 7.5, 4, init_latent=x_T)
        k = s.last_call_stats()["kernels"]
        return lat, k, s.sample_image(ctx, unc, 7.5, 4, init_latent=x_T)

    fresh = _new_sd(d, synth, *FINAL)     # never sees a new entry point
    try:
        ref = plain(fresh)
    finally:
        fresh.close()
    before = plain(sd)
    good = sd.sample_latent_hires(ctx, unc, 7.5, 3, BASE, 0.5, hires_steps=4, init_latent=x_base, hires_seed=1)
    assert sd.latent_size == FINAL
    after = plain(sd)
    for got in (before, after):
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2])
    # failed hires calls: SDMI_ERR_INVALID, the size stays, the next good call gives the same bits
    F = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    out = np.empty((n, 4, *FINAL), np.float32)

    def call(n_steps=3, **kw):
        hr = SdmiHires()
        hr.base_h, hr.base_w, hr.mode, hr.antialias, hr.hires_steps, hr.strength, hr.hires_seed = 8, 8, 2, 0, 4, 0.5, 1
        for k, v in kw.items():
            setattr(hr, k, v)
        return sd._lib.sdmi_hires_latent(sd._ctx, F(ctx), n, 7, F(unc), 3, 7.5, n_steps, F(x_base), 0, C.byref(hr), None, F(out))

    assert call() == 0 and np.array_equal(out, good)
    bad = [dict(base_h=12), dict(base_w=0), dict(base_h=-8), dict(mode=3), dict(mode=-1), dict(mode=0, antialias=1), dict(strength=0.0),
           dict(strength=1.0001), dict(strength=float("nan")), dict(strength=0.1), dict(hires_steps=-1), dict(hires_steps=1001)]
    for kw in bad:
        assert call(**kw) == SDMI_ERR_INVALID, kw
        assert sd.latent_size == FINAL
    assert call(n_steps=0) == SDMI_ERR_INVALID and call(n_steps=1001) == SDMI_ERR_INVALID and sd.latent_size == FINAL
    assert sd._lib.sdmi_hires_latent(sd._ctx, F(ctx), n, 7, F(unc), 3, 7.5, 3, F(x_base), 0, None, None, F(out)) == SDMI_ERR_INVALID
    assert call() == 0 and np.array_equal(out, good)
    last = plain(sd)
    assert np.array_equal(last[0], ref[0]) and last[1] == ref[1] and np.array_equal(last[2], ref[2])
