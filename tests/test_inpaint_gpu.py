"""A UNet with conditioning channels and the SD v1 inpainting checkpoints on the GPU (include/sdmi.h "a UNet with conditioning channels"; DESIGN.md section
9f), through the C ABI, against the CPU restatement in tests/inpaint_ref.py.  Every bar is a neighbouring module's: test_views_gpu (operator level),
test_img2img_gpu (fp32 latents, 1 LSB on the u8 image), test_bf16_gpu / test_fp8_gpu (relative RMS at precision 1 / 2), test_encoder_gpu (the encoder)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import img2img_ref as R
import inpaint_ref as IR
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
ENCODER_BAR = 5e-5         # tests/test_encoder_gpu.py test_encode_image_tiny
F = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))     # noqa: E731
U8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))    # noqa: E731


def _make(d, unet_in_ch, precision=0, **kw):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    return StableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision, unet_in_ch=unet_in_ch, **kw))


@pytest.fixture(scope="module")
def sd9(tiny_dims, synth):
    sd = _make(tiny_dims, 9)
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture(scope="module")
def sd8(tiny_dims, synth):
    sd = _make(tiny_dims, 8)
    sd.load_weights(synth, clip=False)
    yield sd
    sd.close()


@pytest.fixture(scope="module", params=[1, 2])
def sd9_lowp(request, synth):
    sd = _make(BF16_DIMS, 9, request.param)
    sd.load_weights(synth, clip=False)
    if request.param == 2:
        sd.set_option("fp8_min_rows", 1)     # 16 x 16 latents have few rows per GEMM: the MXFP8 path anyway (tests/test_fp8_gpu.py)
    yield sd, request.param
    sd.close()


def _inputs(d, n, T, Tu, cond_ch, seed=0):
    ctx = np.stack([syn.cond_context(i, T, d.ctx_dim) for i in range(n)])
    unc = syn.uncond_context(Tu, d.ctx_dim)
    rng = np.random.default_rng(700 + seed)
    z0 = (rng.standard_normal((n, 4, d.latent_h, d.latent_w)) * 0.8).astype(np.float32)
    noise = np.stack([syn.initial_latent(10 + i, d.latent_h, d.latent_w) for i in range(n)])
    cond = rng.standard_normal((n, cond_ch, d.latent_h, d.latent_w)).astype(np.float32)
    if cond_ch == 5:
        cond[:, 0] = (cond[:, 0] > 0)     # a mask channel of 0 / 1, as the inpainting rule gives
    return ctx, unc, z0, noise, cond


def _picture(d, n, seed=0):
    """an init picture and a pixel mask with the values 0, 127, 128, 255 and edges off the 8-pixel grid"""
    rng = np.random.default_rng(800 + seed)
    H, Wd = 8 * d.latent_h, 8 * d.latent_w
    img = rng.integers(0, 256, (n, H, Wd, 3), dtype=np.uint8)
    mask = np.zeros((n, H, Wd), np.uint8)
    mask[:, 13:H - 27, 21:Wd - 35] = 255
    mask[:, 40:51, 30:70] = 128
    mask[:, 60:67, 30:70] = 127
    if n > 1:
        mask[1] = np.roll(mask[0], (16, -24), (0, 1))
    return img, mask


def _rel_rms(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.sqrt(np.mean((got - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


# ---- 1. the convolutions the feature leans on -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ops16():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion(ModelConfig(64, 1, 64, 8, 8, 64, precision=1))
    yield sd
    sd.close()


@pytest.mark.parametrize("cin", [12, 8])
def test_conv2d_small_cin(sd_ops, ops16, cin):
    g = np.random.default_rng(cin)
    x = g.standard_normal((2, cin, 16, 16)).astype(np.float32)
    w = (g.standard_normal((160, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    b = g.standard_normal(160).astype(np.float32)
    ref = torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1).numpy()
    _check(sd_ops.op_conv2d(x, w, b), ref, f"fp32 conv cin={cin}", FP32_BAR)
    _check(ops16.op_conv2d(x, w, b), ref, f"bf16 conv cin={cin}", BF16_BAR)


# ---- 2. sdmi_unet_forward_cond ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [999, 1])
@pytest.mark.parametrize("ch", [9, 8])
def test_unet_forward_cond(sd9, sd8, synth, tiny_dims, ch, t):
    d, sd = tiny_dims, (sd9 if ch == 9 else sd8)
    ctx, _, lat, _, cond = _inputs(d, 2, 7, 2, ch - 4, seed=ch)
    got = sd.unet.forward(lat, [t], ctx, cond=cond)
    x = torch.from_numpy(np.concatenate([lat, cond], 1))
    refs = [IR.CondUNetOracle(synth, d, dt, ch).forward(x, t, torch.from_numpy(ctx)).numpy() for dt in (torch.float32, torch.float64)]
    e64, e32 = _assert_close(got, refs[0], refs[1], f"unet_forward_cond unet_in_ch={ch} t={t}")
    print(f"unet_forward_cond ch={ch} t={t}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    # one x and one context for both samples: the outputs differ through cond alone, and swapping the cond rows swaps them
    lat1, ctx1 = np.repeat(lat[:1], 2, 0), np.repeat(ctx[:1], 2, 0)
    a = sd.unet.forward(lat1, [t], ctx1, cond=cond)
    b = sd.unet.forward(lat1, [t], ctx1, cond=np.ascontiguousarray(cond[::-1]))
    assert np.abs(a[0] - a[1]).max() > 1e-3, "the conditioning does not reach the output"
    assert np.abs(b - a[::-1]).max() <= 1e-5 * max(1.0, np.abs(a).max())


@functools.lru_cache(maxsize=None)
def _wide_forward64(t):
    d = BF16_DIMS
    ctx, _, lat, _, cond = _inputs(d, 2, 7, 2, 5, seed=20)
    x = torch.from_numpy(np.concatenate([lat, cond], 1))
    return IR.CondUNetOracle(syn.SyntheticWeights(), d, torch.float64, 9).forward(x, t, torch.from_numpy(ctx)).numpy()


@pytest.mark.parametrize("t", [999, 1])
def test_unet_forward_cond_low_precision(sd9_lowp, t):
    sd, precision = sd9_lowp
    ctx, _, lat, _, cond = _inputs(BF16_DIMS, 2, 7, 2, 5, seed=20)
    got = sd.unet.forward(lat, [t], ctx, cond=cond)
    r = _rel_rms(got, _wide_forward64(t))
    print(f"unet_forward_cond precision {precision} t={t}: rel-RMS vs fp64 = {r:.3e}")
    assert np.isfinite(got).all() and r < (BAR_UNET if precision == 1 else BAR_UNET_FP8)


# ---- 3. sdmi_img2img_latent_cond ---------------------------------------------------------------------------------------------------------------------
def _half_mask(n, h, w):
    m = np.zeros((n, 1, h, w), np.float32)
    m[..., : w // 2 - 1] = 1.0
    m[..., w // 2 - 1] = 0.75
    m[..., w // 2] = 0.25
    return m


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("strength", [0.5, 1.0])
def test_img2img_latent_cond(sd9, synth, tiny_dims, strength, masked):
    d = tiny_dims
    ctx, unc, z0, noise, cond = _inputs(d, 2, 7, 3, 5, seed=1)
    mask = _half_mask(2, d.latent_h, d.latent_w) if masked else None
    got = sd9.sample_latent_from(ctx, unc, 7.5, 4, strength, z0, mask=mask, noise=noise, cond=cond)
    a = syn.alphas_cumprod()
    refs = [IR.sample_latent_from(IR.CondUNetOracle(synth, d, dt, 9), a, ctx, unc, 7.5, 4, strength, z0, noise, cond, mask).numpy() for dt in (torch.float32, torch.float64)]
    e64, e32 = _assert_close(got, refs[0], refs[1], f"img2img_latent_cond strength={strength} masked={masked}")
    print(f"img2img_latent_cond strength={strength} masked={masked}: |gpu-f64|={e64:.2e} |f32-f64|={e32:.2e}")
    if masked:
        assert np.array_equal(got[..., -1], z0[..., -1])


def test_img2img_latent_cond_dpmpp_2m(sd9, synth, tiny_dims):
    """the sampler-choice branch of the loop: every forward still reads [x | cond]"""
    d = tiny_dims
    ctx, unc, z0, noise, cond = _inputs(d, 2, 7, 3, 5, seed=2)
    try:
        sd9.set_sampler("dpmpp_2m")
        got = sd9.sample_latent_from(ctx, unc, 7.5, 4, 1.0, z0, noise=noise, cond=cond)
    finally:
        sd9.set_sampler(None)
    a = syn.alphas_cumprod()
    ts, step = R.timesteps(4, 1.0)
    a0 = float(a[ts[0]])
    refs = []
    for dt in (torch.float32, torch.float64):
        unet = IR.CondUNetOracle(synth, d, dt, 9)
        c, u, k = (torch.from_numpy(v).to(dt) for v in (ctx, unc, cond))
        x = (np.sqrt(a0) * torch.from_numpy(z0).to(dt) + np.sqrt(1.0 - a0) * torch.from_numpy(noise).to(dt))
        with torch.no_grad():
            refs.append(SR.sample_textbook("dpmpp_2m", 0.0, a, ts, step, x, lambda x_, t, cur: IR.forward_diffuser(unet, x_, t, c, u, 7.5, k)).numpy())
    _assert_close(got, refs[0], refs[1], "img2img_latent_cond dpmpp_2m")


def test_img2img_latent_cond_dev_equals_host(sd9, tiny_dims):
    d, n = tiny_dims, 2
    ctx, unc, z0, noise, cond = _inputs(d, n, 7, 3, 5, seed=3)
    mask = _half_mask(n, d.latent_h, d.latent_w)
    host = sd9.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=mask, noise=noise, cond=cond)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(ctx=ctx, unc=unc, z0=z0, noise=noise, mask=mask, cond=cond).items()}
    lat = torch.empty((n, 4, d.latent_h, d.latent_w), dtype=torch.float32, device="cuda")
    st = sd9._lib.sdmi_img2img_latent_cond_dev(sd9._ctx, t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["z0"].data_ptr(), t["mask"].data_ptr(),
                                               t["noise"].data_ptr(), 0, t["cond"].data_ptr(), lat.data_ptr())
    assert st == 0
    assert np.array_equal(lat.cpu().numpy(), host)


def test_img2img_latent_cond_precision_1(sd9_lowp):
    sd, precision = sd9_lowp
    if precision != 1:
        return      # the latent bar of precision 1 (tests/test_bf16_gpu.py BAR_LATENT) is the one this project has
    d = BF16_DIMS
    ctx, unc, z0, noise, cond = _inputs(d, 1, 7, 3, 5, seed=4)
    got = sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=noise, cond=cond)
    ref = IR.sample_latent_from(IR.CondUNetOracle(syn.SyntheticWeights(), d, torch.float64, 9), syn.alphas_cumprod(), ctx, unc, 7.5, 4, 0.5, z0, noise, cond).numpy()
    r = _rel_rms(got, ref)
    print(f"img2img_latent_cond precision 1: rel-RMS vs fp64 = {r:.3e}")
    assert np.isfinite(got).all() and r < BAR_LATENT


# ---- 4. sdmi_inpaint_cond ------------------------------------------------------------------------------------------------------------------------------
def test_inpaint_cond(sd9, synth, tiny_dims):
    from stable_diffusion_burn_amd import inpaint_latent_mask
    d = tiny_dims
    img, mask = _picture(d, 2)
    assert {0, 127, 128, 255} <= set(np.unique(mask))
    got = sd9.inpaint_cond(img, mask)
    ref = IR.inpaint_cond(O.EncoderOracle(synth, d, torch.float64), img, mask).numpy()
    assert np.array_equal(got[:, 0], ref[:, 0].astype(np.float32)), "mask channel"
    assert np.array_equal(got[:, 0], inpaint_latent_mask(mask, d.latent_h, d.latent_w))
    assert 0 < got[:, 0].mean() < 1
    _check(got[:, 1:] / R.VAE_SCALE, ref[:, 1:] / 0.18215, "inpaint_cond encoded channels", ENCODER_BAR)
    # and it is the composition of the public encoder call on the masked picture
    z = sd9.autoencoder.encode_image(IR.masked_input(img, mask)) * R.VAE_SCALE
    assert np.array_equal(got[:, 1:], z)


# ---- 5. sdmi_inpaint_image -----------------------------------------------------------------------------------------------------------------------------
def test_inpaint_image(sd9, synth, tiny_dims):
    from stable_diffusion_burn_amd import inpaint_latent_mask
    d, n = tiny_dims, 2
    ctx, unc, _, noise, _ = _inputs(d, n, 7, 3, 5, seed=5)
    img, mask = _picture(d, n, seed=1)
    got = sd9.inpaint_image(ctx, unc, 7.5, 4, 0.75, img, mask, noise=noise)
    cond = sd9.inpaint_cond(img, mask)
    z0 = sd9.autoencoder.encode_image(R.rgb_to_model_input(img)) * R.VAE_SCALE
    lat = sd9.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, noise=noise, cond=cond)
    assert np.array_equal(sd9.latent_to_image(lat), got), "inpaint_image != the composition of the public calls"
    # paste_back
    pasted = sd9.inpaint_image(ctx, unc, 7.5, 4, 0.75, img, mask, paste_back=True, noise=noise)
    keep = mask < 128
    assert np.array_equal(pasted[keep], img[keep]) and np.array_equal(pasted[~keep], got[~keep])
    # latent_blend = the composition with mask = the latent mask
    lm = inpaint_latent_mask(mask, d.latent_h, d.latent_w)
    blended = sd9.inpaint_image(ctx, unc, 7.5, 4, 0.75, img, mask, latent_blend=True, noise=noise)
    lat_b = sd9.sample_latent_from(ctx, unc, 7.5, 4, 0.75, z0, mask=lm, noise=noise, cond=cond)
    assert np.array_equal(sd9.latent_to_image(lat_b), blended)
    assert not np.array_equal(blended, got)
    # the fp64 reference
    o64 = O.StableDiffusionOracle(synth, syn.alphas_cumprod(), d, torch.float64)
    enc = O.EncoderOracle(synth, d, torch.float64)
    ref_lat = IR.sample_latent_from(IR.CondUNetOracle(synth, d, torch.float64, 9), syn.alphas_cumprod(), ctx, unc, 7.5, 4, 0.75, R.encode_z0(enc, img), noise,
                                    IR.inpaint_cond(enc, img, mask))
    ref_img, _ = o64.latent_to_image(ref_lat)
    di = int(np.abs(got.astype(np.int16) - ref_img.astype(np.int16)).max())
    print(f"inpaint_image: u8 max diff {di} LSB")
    assert di <= 1
    # device pointers
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(ctx=ctx, unc=unc, img=img, mask=mask, noise=noise).items()}
    rgb = torch.empty((n, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=torch.uint8, device="cuda")
    from stable_diffusion_burn_amd._capi import SdmiInpaint
    opt = SdmiInpaint(latent_blend=0, paste_back=1)
    st = sd9._lib.sdmi_inpaint_image_dev(sd9._ctx, t["ctx"].data_ptr(), n, 7, t["unc"].data_ptr(), 3, 7.5, 4, 0.75, t["img"].data_ptr(), t["mask"].data_ptr(),
                                         C.byref(opt), t["noise"].data_ptr(), 0, rgb.data_ptr())
    assert st == 0 and np.array_equal(rgb.cpu().numpy(), pasted)


# ---- 6. loaders --------------------------------------------------------------------------------------------------------------------------------------------
def _probe(sd, d):
    ctx, _, lat, _, cond = _inputs(d, 1, 7, 2, 5, seed=6)
    return sd.unet.forward(lat, [500], ctx, cond=cond)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("how", ["safetensors_f16", "dump_tree", "flat_pack"])
def test_loaders(sd9, synth, tiny_dims, tmp_path, how):
    d = tiny_dims
    specs = sd9.weight_specs()
    shapes = dict(specs)
    assert shapes["unet/input_blocks/conv/weight"] == (d.model_channels, 9, 3, 3)
    rnd = (lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)) if how == "safetensors_f16" else (lambda a: a)
    get = lambda n, s: syn.named_tensor(synth, n, s, shapes)     # noqa: E731
    A, B = _make(d, 9), _make(d, 9)
    try:
        A.set_option("keep_masters", 1)
        if how == "safetensors_f16":
            path = tmp_path / "inpaint.safetensors"
            W.write_checkpoint_safetensors(path, specs, get, syn.alphas_cumprod(1000), dtype="F16")
            A.load_weights_safetensors(path)
        elif how == "dump_tree":
            W.write_dump_tree(tmp_path / "dump", specs, get, syn.alphas_cumprod(1000), n_head=d.n_head)
            A.load_weights_dir(str(tmp_path / "dump"))
        else:
            A.load_weights_packed(A.pack_weights(synth, groups=5), groups=5)
        for name, shape in specs:
            B.set_weight(name, syn.alphas_cumprod(1000) if name == "alphas_cumprod" else rnd(get(name, shape)))
        assert B._lib.sdmi_finalize_weights(B._ctx) == 0
        a, b = _probe(A, d), _probe(B, d)
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(_bits(a), _bits(b))
        if how == "flat_pack":
            assert np.array_equal(_bits(a), _bits(_probe(sd9, d)))
        # the unpadded tensor comes back; a LoRA target on the padded conv_in is refused
        w = A.effective_weight("unet/input_blocks/conv/weight")
        assert w.shape == (d.model_channels, 9, 3, 3) and np.array_equal(_bits(w), _bits(rnd(get("unet/input_blocks/conv/weight", w.shape))))
    finally:
        A.close()
        B.close()


def test_lora_on_conv_in(synth, tiny_dims):
    from stable_diffusion_burn_amd import SdmiError
    d = tiny_dims
    for ch, status in ((9, SDMI_ERR_UNSUPPORTED), (8, 0)):
        sd = _make(d, ch)
        try:
            sd.set_option("keep_masters", 1)
            sd.load_weights(synth, clip=False, vae_encoder=False)
            g = np.random.default_rng(ch)
            t = {"unet/input_blocks/conv/weight": (g.standard_normal((2, ch, 3, 3)).astype(np.float32), g.standard_normal((d.model_channels, 2)).astype(np.float32), 1.0)}
            if status:
                with pytest.raises(SdmiError) as ei:
                    sd.lora_attach(t)
                assert ei.value.status == status
            else:
                ad = sd.lora_attach(t, scale=0.5)
                w = sd.effective_weight("unet/input_blocks/conv/weight")
                assert w.shape == (d.model_channels, 8, 3, 3) and np.isfinite(w).all()
                ad.detach()
        finally:
            sd.close()


@pytest.mark.parametrize("dtype", ["F32", "F16", "BF16"])
def test_unpack_pad_transform(sd_ops, dtype):
    g = np.random.default_rng(11)
    for shape in ((8, 9, 3, 3), (8, 3, 3, 3), (5, 7, 1, 1)):
        x = g.standard_normal(shape).astype(np.float32)
        if dtype == "F16":
            raw = x.astype(np.float16)
            want = raw.astype(np.float32)
        elif dtype == "BF16":
            raw = W.bf16_bits(x)
            want = W.bf16_to_f32(raw)
        else:
            raw = want = x
        pc = (shape[1] + 3) // 4 * 4
        ref = np.zeros((shape[0], pc) + shape[2:], np.float32)
        ref[:, :shape[1]] = want
        got = sd_ops.op_unpack_tensor(raw, dtype, 2)
        assert got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (dtype, shape)


def test_wrong_channel_count_is_refused(sd9, sd_tiny, synth, tiny_dims, tmp_path):
    from stable_diffusion_burn_amd import SdmiError
    d = tiny_dims
    files = {}
    for sd, ch in ((sd9, 9), (sd_tiny, 4)):
        specs = [(n, s) for n, s in sd.weight_specs() if sd._group_of(n) == sd.GROUP_HOT]
        shapes = dict(sd.weight_specs())
        files[ch] = tmp_path / f"ch{ch}.safetensors"
        W.write_checkpoint_safetensors(files[ch], specs, lambda n, s: syn.named_tensor(synth, n, s, shapes), syn.alphas_cumprod(1000), dtype="F16")
    ctx, _, lat, _, cond = _inputs(d, 1, 7, 2, 5, seed=7)
    before9, before4 = sd9.unet.forward(lat, [500], ctx, cond=cond), sd_tiny.unet.forward(lat, [500], ctx)
    for sd, other in ((sd_tiny, 9), (sd9, 4)):
        with pytest.raises(SdmiError) as ei:
            sd.load_weights_safetensors(files[other])
        assert ei.value.status == SDMI_ERR_WEIGHTS
        msg = str(ei.value)
        assert "model.diffusion_model.input_blocks.0.0.weight" in msg and f",{other},3,3]" in msg and f",{13 - other},3,3]" in msg, msg
    assert np.array_equal(_bits(sd9.unet.forward(lat, [500], ctx, cond=cond)), _bits(before9))
    assert np.array_equal(_bits(sd_tiny.unet.forward(lat, [500], ctx)), _bits(before4))


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------------------------
def test_statuses(sd9, sd8, sd_tiny, tiny_dims):
    from stable_diffusion_burn_amd import ModelConfig, SdmiError, StableDiffusion
    from stable_diffusion_burn_amd._capi import SdmiConfig, SdmiHires
    d, lib = tiny_dims, sd9._lib
    h, w = d.latent_h, d.latent_w
    ctx, unc, z0, noise, cond = _inputs(d, 1, 7, 2, 5, seed=8)
    img, mask = _picture(d, 1)
    out, rgb, cond_out = np.empty_like(z0), np.empty_like(img), np.empty((1, 5, h, w), np.float32)
    good9 = sd9.unet.forward(z0, [500], ctx, cond=cond)
    good4 = sd_tiny.unet.forward(z0, [500], ctx)

    def status_of(fn):
        st = fn()
        return st, lib.sdmi_last_error().decode()

    # a conditioned context answers the entries that take no cond with SDMI_ERR_STATE, naming the _cond entry
    hr = SdmiHires(base_h=8, base_w=8, mode=1, antialias=0, hires_steps=0, strength=0.5, hires_seed=0)
    plain_calls = {
        "unet_forward": lambda c: lib.sdmi_unet_forward(c, F(z0), 500, F(ctx), 1, 7, F(out)),
        "sample_latent": lambda c: lib.sdmi_sample_latent(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, F(noise), 0, F(out)),
        "sample_image": lambda c: lib.sdmi_sample_image(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, F(noise), 0, U8(rgb)),
        "img2img_latent": lambda c: lib.sdmi_img2img_latent(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, 1.0, F(z0), None, F(noise), 0, F(out)),
        "img2img_image": lambda c: lib.sdmi_img2img_image(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, 1.0, U8(img), None, F(noise), 0, U8(rgb)),
        "hires_latent": lambda c: lib.sdmi_hires_latent(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, None, 0, C.byref(hr), None, F(out)),
        "hires_image": lambda c: lib.sdmi_hires_image(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, None, 0, C.byref(hr), None, U8(rgb)),
    }
    for name, call in plain_calls.items():
        for sd in (sd9, sd8):
            st, msg = status_of(lambda: call(sd._ctx))
            assert st == SDMI_ERR_STATE and "_cond" in msg, (name, st, msg)
        assert call(sd_tiny._ctx) == 0, name
    # the _cond entries and sdmi_inpaint_* on a 4-channel context; sdmi_inpaint_* where unet_in_ch != 9
    cond_calls = {
        "unet_forward_cond": lambda c, k: lib.sdmi_unet_forward_cond(c, F(z0), 500, F(ctx), k, 1, 7, F(out)),
        "img2img_latent_cond": lambda c, k: lib.sdmi_img2img_latent_cond(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, 1.0, F(z0), None, F(noise), 0, k, F(out)),
    }
    for name, call in cond_calls.items():
        assert call(sd_tiny._ctx, F(cond)) == SDMI_ERR_STATE, name
        assert call(sd9._ctx, None) == SDMI_ERR_INVALID, name
        assert call(sd9._ctx, F(cond)) == 0, name
    inpaint_calls = {
        "inpaint_cond": lambda c: lib.sdmi_inpaint_cond(c, U8(img), U8(mask), 1, F(cond_out)),
        "inpaint_image": lambda c: lib.sdmi_inpaint_image(c, F(ctx), 1, 7, F(unc), 2, 7.5, 2, 1.0, U8(img), U8(mask), None, F(noise), 0, U8(rgb)),
    }
    for name, call in inpaint_calls.items():
        assert call(sd_tiny._ctx) == SDMI_ERR_STATE, name
        assert call(sd8._ctx) == SDMI_ERR_STATE, name
        assert call(sd9._ctx) == 0, name
    assert lib.sdmi_inpaint_cond(sd9._ctx, None, U8(mask), 1, F(cond_out)) == SDMI_ERR_INVALID
    assert lib.sdmi_inpaint_image(sd9._ctx, F(ctx), 1, 7, F(unc), 2, 7.5, 2, 1.0, U8(img), None, None, F(noise), 0, U8(rgb)) == SDMI_ERR_INVALID
    # unet_in_ch outside {0, 4 .. 12}
    for ch, want in ((3, SDMI_ERR_INVALID), (13, SDMI_ERR_INVALID), (-1, SDMI_ERR_INVALID), (0, 0), (12, 0)):
        cfg = SdmiConfig()
        assert lib.sdmi_default_config(C.byref(cfg)) == 0
        cfg.model_channels, cfg.n_head, cfg.ctx_dim, cfg.latent_h, cfg.latent_w, cfg.vae_ch, cfg.clip_layers = 32, 1, 32, 8, 8, 32, 0
        cfg.unet_in_ch = ch
        c = C.c_void_p()
        assert lib.sdmi_create(C.byref(c), C.byref(cfg)) == want, ch
        if want == 0:
            dims = (C.c_int64 * 4)()
            name, nd = C.c_char_p(), C.c_int32()
            shapes = {}
            for i in range(lib.sdmi_weight_count(c)):
                assert lib.sdmi_weight_info(c, i, C.byref(name), C.byref(nd), dims) == 0
                shapes[name.value.decode()] = tuple(dims[k] for k in range(nd.value))
            assert shapes["unet/input_blocks/conv/weight"] == (32, ch or 4, 3, 3)
            lib.sdmi_destroy(c)
    # the sharded path
    from stable_diffusion_burn_amd import MultiStableDiffusion
    m = MultiStableDiffusion(ModelConfig(d.model_channels, d.n_head, d.ctx_dim, h, w, d.vae_ch, unet_in_ch=9), devices=(0,))
    try:
        with pytest.raises(SdmiError) as ei:
            m.sample_image(ctx[0], unc, 7.5, 2, 1, init_latents=noise)
        assert ei.value.status == SDMI_ERR_UNSUPPORTED
    finally:
        m.close()
    # after all of it the contexts still run, to the same bits
    assert np.array_equal(_bits(sd9.unet.forward(z0, [500], ctx, cond=cond)), _bits(good9))
    assert np.array_equal(_bits(sd_tiny.unet.forward(z0, [500], ctx)), _bits(good4))


# ---- 8. pool_fill ---------------------------------------------------------------------------------------------------------------------------------------------
def test_pool_fill(sd9, tiny_dims, tmp_path):
    """the pad channels of the assembled UNet input (and of the cond rows) are written on every launch: the padded conv_in weights are zero there, and 0 x NaN is NaN"""
    d = tiny_dims
    ctx, unc, z0, noise, cond = _inputs(d, 2, 7, 2, 5, seed=9)
    img, mask = _picture(d, 1, seed=2)
    _sweep(sd9, tmp_path, lambda: sd9.unet.forward(z0, [500], ctx, cond=cond), "unet_forward_cond unet_in_ch=9")
    _sweep(sd9, tmp_path, lambda: sd9.inpaint_image(ctx[:1], unc, 7.5, 2, 1.0, img, mask, latent_blend=True, paste_back=True, noise=noise[:1]), "inpaint_image unet_in_ch=9")
    try:
        sd9.set_option("pool_fill", 0xFF)
        _fills(sd9, tmp_path)
        sd9.unet.forward(z0, [500], ctx, cond=cond)
        assert _fills(sd9, tmp_path)[0] > 0
    finally:
        sd9.set_option("pool_fill", -1)


# ---- 9. profile -------------------------------------------------------------------------------------------------------------------------------------------------
def test_profile_class_and_launch_count(sd9, sd_tiny, tiny_dims):
    """Class 8 ("other") of a k-step sdmi_img2img_latent_cond at precision 0 with the default sampler and no mask, from engine.cpp: timestep embedding 1 + SiLU 2
    (unet_prepare), the start latent 1, the cond layout conversion 1, per step the input assembly 1, the two duplications of the CFG pair's shared prefix in
    front of the first cross attention (spatial_transformer, option cfg_share) and the CFG + DDIM update 1, the NCHW conversion of the result 1: 4 k + 6.  The
    same call on a 4-channel context: 3 k + 5.  The two contexts run the same launch list otherwise, except for what the GEMM planner makes of
    conv_in's K = 108 against 36 (its kernel class, a split-K reduce): so last_call_stats of the conditioned call has exactly k + 1 launches -- k assemblies and
    the one layout conversion -- more than the same call has without them, once the GEMM classes' own difference is taken out."""
    d = tiny_dims
    ctx, unc, z0, noise, cond = _inputs(d, 1, 7, 2, 5, seed=10)
    gemm_classes = ("conv_gemm", "splitk_reduce", "conv_gemm_split")
    for k in (2, 4):
        stats = {}
        for name, sd, kw in (("cond", sd9, {"cond": cond}), ("plain", sd_tiny, {})):
            try:
                sd.set_option("profile", 1)
                sd.set_option("profile_reset", 1)
                sd.sample_latent_from(ctx, unc, 7.5, k, 1.0, z0, noise=noise, **kw)
                stats[name] = ({c: v["launches"] for c, v in sd.profile_stats().items()}, sd.last_call_stats()["kernels"])
                assert sd.profile_stats()["other"]["ms"] > 0
            finally:
                sd.set_option("profile", 0)
        (pc, kc), (pp, kp) = stats["cond"], stats["plain"]
        assert set(gemm_classes) <= set(pc), sorted(pc)
        assert pc["other"] == 4 * k + 6 and pp["other"] == 3 * k + 5, (k, pc, pp)
        for c in pc:
            if c != "other" and c not in gemm_classes:
                assert pc[c] == pp[c], (c, pc, pp)
        gemm_diff = sum(pc[c] - pp[c] for c in gemm_classes)
        print(f"k={k}: launches {kc} conditioned, {kp} plain; GEMM classes differ by {gemm_diff}")
        assert kc - kp == (k + 1) + gemm_diff, (k, kc, kp, pc, pp)
