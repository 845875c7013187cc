"""img2img on the host (no GPU): the schedule entry sdmi_img2img_timesteps against rule 1, the CPU restatement
against the oracle's sampler, the Rust shim's declarations and the new code object."""
import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import img2img_ref as R
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

ROOT = Path(__file__).resolve().parents[1]
BUILD = ROOT / "stable_diffusion_burn_amd" / "build"
LLVM = Path("/opt/rocm/lib/llvm/bin")
SDMI_ERR_INVALID = -1
NEW_SYMBOLS = ["sdmi_img2img_timesteps", "sdmi_img2img_latent", "sdmi_img2img_image", "sdmi_img2img_latent_dev", "sdmi_img2img_image_dev"]


@pytest.fixture(scope="module")
def lib():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    from stable_diffusion_burn_amd import _capi
    return _capi.load_library()


def _timesteps(lib, total, n_steps, strength, capacity=1000):
    buf = (C.c_int32 * max(1, capacity))()
    count = C.c_int32(-7)
    st = lib.sdmi_img2img_timesteps(total, n_steps, strength, buf, capacity, C.byref(count))
    return st, list(buf[:max(0, count.value)]) if st == 0 else None, count.value


def test_new_symbols_exported(lib):
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s


@pytest.mark.parametrize("n_steps", [1, 3, 20, 30, 50, 1000])
@pytest.mark.parametrize("strength", [0.05, 0.3, 0.5, 0.75, 0.999, 1.0])
def test_timesteps_match_rule_1(lib, n_steps, strength):
    ts, step = O.ddim_timesteps(n_steps, 1000)
    L = len(ts)
    k = min(L, int(strength * L))
    st, got, count = _timesteps(lib, 1000, n_steps, strength)
    if k < 1:
        assert st == SDMI_ERR_INVALID
        return
    assert st == 0 and count == k
    assert got == ts[L - k:]
    assert got == R.timesteps(n_steps, strength)[0]
    if n_steps == 30 and strength == 1.0:
        assert count == 31   # quirk Q5: 1000 // 30 = 33 -> 999, 966, ..., 9: 31 entries


def test_timesteps_python_entry_point(lib):
    from stable_diffusion_burn_amd import img2img_timesteps
    assert img2img_timesteps(20, 0.5) == [499, 449, 399, 349, 299, 249, 199, 149, 99, 49]
    assert img2img_timesteps(1, 1.0) == [999]
    assert img2img_timesteps(4, 0.5, total=100) == [49, 24]


@pytest.mark.parametrize("strength", [0.0, -0.1, 1.0001, float("nan")])
def test_timesteps_reject_bad_strength(lib, strength):
    st, _, _ = _timesteps(lib, 1000, 20, strength)
    assert st == SDMI_ERR_INVALID
    assert b"strength" in lib.sdmi_last_error()


def test_timesteps_reject_less_than_one_step(lib):
    assert _timesteps(lib, 1000, 20, 0.04)[0] == SDMI_ERR_INVALID   # 0.04 * 20 = 0.8
    assert _timesteps(lib, 1000, 1, 0.999)[0] == SDMI_ERR_INVALID   # L = 1
    assert _timesteps(lib, 1000, 0, 1.0)[0] == SDMI_ERR_INVALID
    assert _timesteps(lib, 1000, 1001, 1.0)[0] == SDMI_ERR_INVALID


def test_timesteps_short_capacity_reports_count(lib):
    st, _, count = _timesteps(lib, 1000, 50, 0.5, capacity=10)
    assert st == SDMI_ERR_INVALID and count == 25
    count = C.c_int32(0)
    assert lib.sdmi_img2img_timesteps(1000, 50, 0.5, None, 0, C.byref(count)) == SDMI_ERR_INVALID and count.value == 25
    assert lib.sdmi_img2img_timesteps(1000, 50, 0.5, None, 0, None) == SDMI_ERR_INVALID


def test_python_layer_validates_before_calling_in(lib):
    """ValueError on shapes and ranges before the C call; without a GPU the object is built around a null context."""
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion.__new__(StableDiffusion)
    sd._lib, sd.config, sd._ctx, sd._owned = lib, ModelConfig(64, 1, 32, 8, 8, 32), C.c_void_p(), True
    ctx, unc = np.zeros((1, 3, 32), np.float32), np.zeros((2, 32), np.float32)
    z0 = np.zeros((1, 4, 8, 8), np.float32)
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            sd.sample_latent_from(ctx, unc, 7.5, 4, bad, z0)
    with pytest.raises(ValueError, match="z0"):
        sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0[:, :3])
    with pytest.raises(ValueError, match="mask"):
        sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, mask=np.ones((1, 4, 4), np.float32))
    with pytest.raises(ValueError, match="noise"):
        sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, noise=np.ones((2, 4, 8, 8), np.float32))
    with pytest.raises(ValueError, match="mask"):
        sd.sample_latent_from(ctx, unc, 7.5, 4, 0.5, z0, mask=np.full((1, 8, 8), 1.5, np.float32))
    with pytest.raises(ValueError, match="init_image"):
        sd.sample_image_from(ctx, unc, 7.5, 4, 0.5, np.zeros((1, 64, 64, 3), np.float32))
    with pytest.raises(ValueError, match="mask"):
        sd.sample_image_from(ctx, unc, 7.5, 4, 0.5, np.zeros((1, 64, 64, 3), np.uint8), mask=np.ones((1, 32, 32), bool))


def test_normal_stream_is_standard_normal():
    x = R.normal_stream(5, 1 << 16)
    assert x.dtype == np.float32 and np.isfinite(x).all()
    assert abs(float(x.mean())) < 0.02 and abs(float(x.std()) - 1.0) < 0.02
    assert not np.array_equal(R.normal_stream(6, 64), x[:64])
    assert np.array_equal(R.seeded_noise(5, 2, 4, 4)[1].ravel(), R.normal_stream(6, 64))


def test_restatement_at_full_strength_is_txt2img():
    """strength = 1 and z0 = 0: x_t0 = sqrt(1 - a_999) eps, then the whole schedule -- exactly the oracle's sample_latent"""
    d = O.Dims(32, 1, 32, 8, 8, 32)
    ora = O.StableDiffusionOracle(syn.SyntheticWeights(), syn.alphas_cumprod(), d, torch.float64)
    ctx = torch.from_numpy(syn.cond_context(0, 5, 32)[None])
    unc = torch.from_numpy(syn.uncond_context(3, 32))
    eps = torch.from_numpy(syn.initial_latent(0, 8, 8)[None]).to(torch.float64)
    z0 = torch.zeros_like(eps)
    a999 = float(syn.alphas_cumprod()[999])
    for n_steps in (1, 2):
        got = R.sample_latent_from(ora, ctx, unc, 7.5, n_steps, 1.0, z0, eps)
        ref = ora.sample_latent(ctx, unc, 7.5, n_steps, math.sqrt(1.0 - a999) * eps)
        assert torch.equal(got, ref), n_steps
        # a mask of zeros ends exactly at z0; of ones changes nothing
        assert torch.equal(R.sample_latent_from(ora, ctx, unc, 7.5, n_steps, 1.0, z0, eps, mask=torch.zeros(1, 1, 8, 8)), z0)
        assert torch.equal(R.sample_latent_from(ora, ctx, unc, 7.5, n_steps, 1.0, z0, eps, mask=torch.ones(1, 1, 8, 8)), ref)


def test_rust_shim_declares_img2img():
    text = (ROOT / "ffi" / "sdmi.rs").read_text()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\bfn {s}\s*\(", text), s
    assert re.search(r"pub fn sample_image_from\s*\(", text)


def test_img2img_code_object_has_no_scratch(lib, tmp_path):
    obj = BUILD / "k_img2img.hip.o"
    assert obj.exists()
    if not (LLVM / "llvm-objdump").exists():
        pytest.skip("needs ROCm's llvm tools")
    fat, dev = tmp_path / "k.fat", tmp_path / "k.co"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(obj), str(tmp_path / "copy.o")], check=True)
    subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                    f"--output={dev}"], check=True)
    text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(dev)], check=True, capture_output=True, text=True).stdout
    funcs = {m.group(1): m.group(2) for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M)}
    kernels = {k: v for k, v in funcs.items() if "kernel" in k}
    assert any("rgb_u8_to_nhwc4" in k for k in kernels) and any("img2img_start" in k for k in kernels)
    assert any("cfg_ddim_masked" in k for k in kernels)
    for name, body in kernels.items():
        assert "scratch_" not in body, f"{name} uses scratch memory"
        assert not re.search(r"^\s*ds_", body, re.M), f"{name} uses LDS"
