"""FreeU (include/sdmi.h "FreeU"), the parts that need no GPU: the closed form the kernel evaluates against the published FFT code, the block
rule against the oracle's topology, the reference forward against the plain oracle, the argument checks and the bindings."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import freeu_ref as FR
from oracle import sd_oracle as O

ROOT = Path(__file__).resolve().parents[1]
SMALL = O.Dims(model_channels=32, n_head=1, ctx_dim=32, latent_h=8, latent_w=8, vae_ch=32)
TINY = O.Dims(model_channels=160, n_head=4, ctx_dim=64, latent_h=16, latent_w=16, vae_ch=32)     # conftest's tiny_dims
NEW_SYMBOLS = ("sdmi_set_freeu", "sdmi_get_freeu", "sdmi_freeu_plan", "sdmi_op_freeu", "sdmi_multi_set_freeu")
SIZES = [(1, 1), (1, 3), (2, 1), (2, 2), (2, 6), (3, 5), (4, 12), (8, 24), (9, 11), (16, 16), (64, 64)]
INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def sdmi():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    import stable_diffusion_burn_amd as pkg
    return pkg


@pytest.mark.parametrize("size", SIZES)
def test_closed_form_is_the_published_filter(size):
    h, w = size
    x = np.random.default_rng(h * 100 + w).standard_normal((2, 3, h, w))
    for s in (0.9, 0.2, 0.0, 1.0, 1.7):
        want, got = FR.fourier_filter(x, s), FR.closed_form(x, s)
        err = np.abs(got - want).max()
        assert err <= 1e-12, f"{size} s={s}: {err:.3e}"
    assert np.array_equal(FR.closed_form(x, 1.0), x)


def test_backbone_versions():
    g = np.random.default_rng(3)
    h = g.standard_normal((2, 8, 3, 5))
    v1 = FR.backbone(h, 1.4, 1)
    assert np.array_equal(v1[:, 4:], h[:, 4:]) and np.allclose(v1[:, :4], 1.4 * h[:, :4], rtol=1e-15)
    v2 = FR.backbone(h, 1.4, 2)
    m = h.mean(axis=1)
    for i in range(2):
        mh = (m[i] - m[i].min()) / (m[i].max() - m[i].min())
        assert np.allclose(v2[i, :4], h[i, :4] * (0.4 * mh + 1.0), rtol=1e-14) and np.array_equal(v2[i, 4:], h[i, 4:])
    # max == min: the published code divides by zero; m_hat = 0 here, so nothing is scaled
    flat = np.ones((1, 8, 2, 2))
    assert np.array_equal(FR.backbone(flat, 1.6, 2), flat)
    one = g.standard_normal((1, 8, 1, 1))
    assert np.array_equal(FR.backbone(one, 1.6, 2), one)


@pytest.mark.parametrize("dims,size", [(O.Dims(), (64, 64)), (O.Dims(), (128, 128)), (TINY, (16, 16)), (TINY, (8, 24))])
def test_plan_is_the_rule_on_the_oracles_topology(sdmi, synth, dims, size):
    want = FR.plan(O.UNetOracle(synth, dims, torch.float64), *size)
    got = sdmi.freeu_plan(dims, *size)
    assert got == want
    mc = dims.model_channels
    assert [g for g, *_ in got] == [1] * 7 + [2] * 3 + [0, 0]
    assert [cx for _, cx, *_ in got] == [4 * mc] * 7 + [2 * mc] * 3 + [mc] * 2
    if size == (8, 24):
        assert got[0][3:] == (1, 3) and got[11][3:] == (8, 24)


def test_plan_refuses_bad_arguments(sdmi):
    from stable_diffusion_burn_amd._capi import SdmiConfig
    lib = sdmi._capi.load_library()
    cfg = SdmiConfig()
    assert lib.sdmi_default_config(C.byref(cfg)) == 0
    out = (C.c_int32 * 60)()
    assert lib.sdmi_freeu_plan(C.byref(cfg), 64, 64, out) == 0 and out[1] == 4 * cfg.model_channels
    assert lib.sdmi_freeu_plan(None, 64, 64, out) == INVALID
    assert lib.sdmi_freeu_plan(C.byref(cfg), 64, 64, None) == INVALID
    assert lib.sdmi_freeu_plan(C.byref(cfg), 60, 64, out) == INVALID
    assert lib.sdmi_freeu_plan(C.byref(cfg), 0, 64, out) == INVALID
    cfg.model_channels = 0
    assert lib.sdmi_freeu_plan(C.byref(cfg), 64, 64, out) == INVALID


def test_symbols_and_bindings(sdmi):
    from stable_diffusion_burn_amd import MultiStableDiffusion, StableDiffusion
    from stable_diffusion_burn_amd._capi import SIGNATURES
    lib = sdmi._capi.load_library()
    header = (ROOT / "include" / "sdmi.h").read_text()
    rs = (ROOT / "ffi" / "sdmi.rs").read_text()
    for s in NEW_SYMBOLS:
        assert s in SIGNATURES and getattr(lib, s).argtypes == SIGNATURES[s][1], s
        assert re.search(rf"\bint {s}\s*\(", header), s
        assert re.search(rf"\bfn {s}\s*\(", rs), s
    for name in ("set_freeu", "get_freeu", "op_freeu"):
        assert callable(getattr(StableDiffusion, name))
    assert callable(MultiStableDiffusion.set_freeu) and callable(sdmi.freeu_plan)


def test_set_freeu_checks_its_arguments_before_the_context(sdmi):
    """every argument error is SDMI_ERR_INVALID with a message of its own, whatever the context -- a null one needs no GPU"""
    lib = sdmi._capi.load_library()
    nan, inf = float("nan"), float("inf")
    bad = [(3, 1.2, 1.4, 0.9, 0.2, 0.0, 1.0), (-1, 1.2, 1.4, 0.9, 0.2, 0.0, 1.0), (1, 0.0, 1.4, 0.9, 0.2, 0.0, 1.0), (1, 1.2, -1.0, 0.9, 0.2, 0.0, 1.0),
           (2, 1.2, 1.4, -0.1, 0.2, 0.0, 1.0), (1, 1.2, 1.4, 0.9, nan, 0.0, 1.0), (1, inf, 1.4, 0.9, 0.2, 0.0, 1.0), (1, 1.2, 1.4, 0.9, 0.2, 0.5, 0.25),
           (1, 1.2, 1.4, 0.9, 0.2, -0.1, 1.0), (1, 1.2, 1.4, 0.9, 0.2, 0.0, 1.5), (1, 1.2, 1.4, 0.9, 0.2, nan, 1.0)]
    for args in bad:
        assert lib.sdmi_set_freeu(None, *args) == INVALID, args
        assert b"freeu" in lib.sdmi_last_error(), args
        assert lib.sdmi_multi_set_freeu(None, *args) == INVALID, args
        assert b"freeu" in lib.sdmi_last_error(), args
    # good values reach the context check
    assert lib.sdmi_set_freeu(None, 1, 1.2, 1.4, 0.9, 0.2, 0.0, 1.0) == INVALID and b"null sdmi_ctx" in lib.sdmi_last_error()
    assert lib.sdmi_set_freeu(None, 0, nan, nan, nan, nan, nan, nan) == INVALID and b"null sdmi_ctx" in lib.sdmi_last_error()   # version 0 ignores the rest
    assert lib.sdmi_get_freeu(None, None, None, None, None, None, None, None) == INVALID
    assert lib.sdmi_op_freeu(None, None, 1, 96, 2, 2, 64, 1, 1.2, 0.9, None, None) == INVALID


def test_cli_refuses_a_bad_SDMI_FREEU_before_anything_is_loaded(sdmi, tmp_path):
    import os
    import subprocess
    cli = ROOT / "stable_diffusion_burn_amd" / "bin" / "sdmi_sample"
    for bad in ("1.2:1.4", "1.2:1.4:0.9:0.2:3", "a:b:c:d", "1.2:1.4:0.9:0.2:2:1", "1.2:1.4:0.9:0.2:"):
        r = subprocess.run([str(cli), "dump", "nowhere", "7.5", "20", "p", "out"], env={**os.environ, "SDMI_FREEU": bad}, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "SDMI_FREEU must be b1:b2:s1:s2[:version]" in r.stderr, (bad, r.stderr)
        assert "Loading" not in r.stdout
    # a good value passes the check: the run gets as far as the tokenizer file it does not have
    r = subprocess.run([str(cli), "dump", "nowhere", "7.5", "20", "p", "out"], env={**os.environ, "SDMI_FREEU": "1.2:1.4:0.9:0.2:2"}, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert "SDMI_FREEU" not in r.stderr and "Loading tokenizer" in r.stdout


def test_reference_forward_with_unit_parameters_is_the_plain_forward(synth):
    d = SMALL
    g = np.random.default_rng(11)
    x = torch.from_numpy(g.standard_normal((2, 4, d.latent_h, d.latent_w)).astype(np.float32))
    ctx = torch.from_numpy(g.standard_normal((2, 5, d.ctx_dim)).astype(np.float32))
    for dtype in (torch.float32, torch.float64):
        unet = O.UNetOracle(synth, d, dtype)
        plain = unet.forward(x, 500, ctx)
        assert torch.equal(FR.freeu_forward(unet, x, 500, ctx, None), plain)
        for version in (1, 2):
            assert torch.equal(FR.freeu_forward(unet, x, 500, ctx, FR.Params(1.0, 1.0, 1.0, 1.0, version)), plain)
    # and the parameters do reach the output
    unet = O.UNetOracle(synth, d, torch.float64)
    plain = unet.forward(x, 500, ctx)
    for p in (FR.Params(1.3, 1.0, 1.0, 1.0), FR.Params(1.0, 1.4, 1.0, 1.0), FR.Params(1.0, 1.0, 0.5, 1.0), FR.Params(1.0, 1.0, 1.0, 0.2), FR.Params(1.3, 1.4, 1.0, 1.0, 2)):
        assert float((FR.freeu_forward(unet, x, 500, ctx, p) - plain).abs().max()) > 1e-6, p
