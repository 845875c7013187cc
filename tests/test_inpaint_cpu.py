"""Conditioned UNet input and inpainting checkpoints (include/sdmi.h "a UNet with conditioning channels"): what needs no GPU -- the
exported surface, the config field, the host-only latent-mask rule against torch, and the CPU restatement (tests/inpaint_ref.py) against itself."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inpaint_ref as IR
from oracle import sd_oracle as O

ROOT = Path(__file__).resolve().parents[1]
SDMI_ERR_INVALID = -1
NEW_SYMBOLS = ["sdmi_unet_forward_cond", "sdmi_img2img_latent_cond", "sdmi_img2img_latent_cond_dev", "sdmi_inpaint_latent_mask", "sdmi_inpaint_cond",
               "sdmi_inpaint_image", "sdmi_inpaint_image_dev"]


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd._capi import load_library
    return load_library()


def test_symbols_exported_and_bound(lib):
    from stable_diffusion_burn_amd import StableDiffusion, UNet, inpaint_latent_mask   # noqa: F401
    from stable_diffusion_burn_amd._capi import SIGNATURES, SdmiInpaint
    header = (ROOT / "include" / "sdmi.h").read_text()
    rs = (ROOT / "ffi" / "sdmi.rs").read_text()
    for s in NEW_SYMBOLS:
        assert s in SIGNATURES and getattr(lib, s).argtypes == SIGNATURES[s][1], s
        assert re.search(rf"\bint {s}\s*\(", header), s
        assert re.search(rf"\bfn {s}\s*\(", rs), s
    assert C.sizeof(SdmiInpaint) == 40
    assert re.search(r"pub struct SdmiInpaint", rs)
    for name in ("inpaint_cond", "inpaint_image"):
        assert callable(getattr(StableDiffusion, name))
    import inspect
    assert "cond" in inspect.signature(UNet.forward).parameters
    assert "cond" in inspect.signature(StableDiffusion.sample_latent_from).parameters


def test_config_field(lib):
    from stable_diffusion_burn_amd import ModelConfig
    from stable_diffusion_burn_amd._capi import SdmiConfig
    cfg = SdmiConfig()
    assert lib.sdmi_default_config(C.byref(cfg)) == 0
    assert cfg.unet_in_ch == 4
    assert C.sizeof(SdmiConfig) == 64
    names = [f[0] for f in SdmiConfig._fields_]
    assert names[-2:] == ["unet_in_ch", "reserved"] and SdmiConfig.unet_in_ch.offset == 52
    assert ModelConfig().unet_in_ch == 4 and ModelConfig(unet_in_ch=9).unet_in_ch == 9


@pytest.mark.parametrize("h,w", [(16, 16), (8, 24)])
def test_latent_mask_is_legacy_nearest(lib, h, w):
    from stable_diffusion_burn_amd import inpaint_latent_mask
    rng = np.random.default_rng(h * 100 + w)
    mask = rng.integers(0, 256, (3, 8 * h, 8 * w), dtype=np.uint8)
    mask[0, ::8, ::16] = 127      # both sides of the threshold on sampled positions
    mask[0, ::8, 8::16] = 128
    mask[1, ::16, ::8] = 128
    mask[1, 8::16, ::8] = 127
    got = inpaint_latent_mask(mask, h, w)
    want = F.interpolate(torch.from_numpy((mask >= 128).astype(np.float32))[:, None], size=(h, w)).numpy()[:, 0]
    assert got.dtype == np.float32 and got.shape == (3, h, w)
    assert np.array_equal(got, want)
    assert set(np.unique(got)) <= {0.0, 1.0} and got[0, 0, 0] == 0.0 and got[0, 0, 1] == 1.0
    # the reference file states the same rule
    assert np.array_equal(IR.latent_mask(mask, h, w), got)
    # and the rule reads mask[8y][8x] alone
    other = mask.copy()
    keep = np.zeros_like(mask, bool)
    keep[:, ::8, ::8] = True
    other[~keep] = 255 - other[~keep]
    assert np.array_equal(inpaint_latent_mask(other, h, w), got)


def test_latent_mask_argument_errors(lib):
    from stable_diffusion_burn_amd import inpaint_latent_mask
    U8 = C.POINTER(C.c_uint8)
    mask = np.zeros((1, 16, 16), np.uint8)
    out = np.zeros((1, 2, 2), np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.sdmi_inpaint_latent_mask(None, 1, 2, 2, fp) == SDMI_ERR_INVALID
    assert lib.sdmi_inpaint_latent_mask(mask.ctypes.data_as(U8), 1, 2, 2, None) == SDMI_ERR_INVALID
    for n, h, w in ((0, 2, 2), (1, 0, 2), (1, 2, -1)):
        assert lib.sdmi_inpaint_latent_mask(mask.ctypes.data_as(U8), n, h, w, fp) == SDMI_ERR_INVALID
    assert lib.sdmi_inpaint_latent_mask(mask.ctypes.data_as(U8), 1, 2, 2, fp) == 0
    # a mask that is not 8x the latent (the C entry takes no mask size: the binding holds the shapes)
    for bad in (np.zeros((1, 16, 17), np.uint8), np.zeros((1, 15, 16), np.uint8), np.zeros((16, 16), np.uint8), np.zeros((1, 16, 16), np.float32)):
        with pytest.raises(ValueError):
            inpaint_latent_mask(bad, 2, 2)


def test_reference_zero_cond_weight_is_the_plain_oracle(synth):
    """a conditioned oracle whose conv_in weight is zero on channels 4 and up equals the plain oracle on x"""
    d = O.Dims(model_channels=32, n_head=1, ctx_dim=32, latent_h=8, latent_w=8, vae_ch=32)
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((2, 4, 8, 8)).astype(np.float32))
    cond = torch.from_numpy(rng.standard_normal((2, 5, 8, 8)).astype(np.float32))
    ctx = torch.from_numpy(rng.standard_normal((2, 3, 32)).astype(np.float32))
    zero = IR.CondUNetOracle(synth, d, torch.float64, unet_in_ch=9, zero_cond=True)
    plain = O.UNetOracle(IR.CondProvider(synth, 9), d, torch.float64)
    a = zero.forward(torch.cat([x, cond], 1), 500, ctx)
    b = plain.forward(x, 500, ctx)
    assert a.shape == (2, 4, 8, 8) and torch.equal(a, b)
    # and the conditioning does reach the output of the full oracle
    full = IR.CondUNetOracle(synth, d, torch.float64, unet_in_ch=9)
    c = full.forward(torch.cat([x, cond], 1), 500, ctx)
    assert (c - a).abs().max() > 1e-3
    c2 = full.forward(torch.cat([x, cond.flip(0)], 1), 500, ctx)
    assert (c2 - c).abs().max() > 1e-3


def test_reference_cond_rule(synth):
    d = O.Dims(model_channels=32, n_head=1, ctx_dim=32, latent_h=8, latent_w=8, vae_ch=32)
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    mask = np.zeros((1, 64, 64), np.uint8)
    mask[:, 10:40, 5:29] = 255
    x = IR.masked_input(img, mask)
    assert np.all(x[:, :, 10:40, 5:29] == 0) and np.array_equal(x[:, :, :10], IR.R.rgb_to_model_input(img)[:, :, :10])
    cond = IR.inpaint_cond(O.EncoderOracle(synth, d, torch.float64), img, mask)
    assert cond.shape == (1, 5, 8, 8)
    assert np.array_equal(cond[:, 0].numpy(), IR.latent_mask(mask, 8, 8))
