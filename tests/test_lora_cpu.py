"""Host side of the LoRA adapters: the float64 merge of tests/lora_ref.py against hand-computed cases, the npz format, the
Python layer's argument checks (against a recording stand-in for the library: nothing may reach it), the bindings, the built merge kernel, and the
oracle's own statement that the adapter of the GPU parity test moves the model by far more than that test's bars."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import synthetic as syn

ROOT = Path(__file__).resolve().parents[1]

BUILD = ROOT / "stable_diffusion_burn_amd" / "build"
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW_SYMBOLS = ["sdmi_lora_create", "sdmi_lora_add", "sdmi_lora_set_scale", "sdmi_lora_get_scale", "sdmi_lora_destroy", "sdmi_lora_effective_weight"]


def test_merge_f64_hand_computed_linear_and_conv():
    """2 x 3, rank 1, both orientations.  Linear weight [in = 2, out = 3]: down [1, 2] = (1, 2), up [3, 1] = (3, 4, 5): delta[i][o] = down[i] up[o].
    Conv weight [cout = 2, cin = 3, 1, 1]: down [1, 3, 1, 1] = (1, 2, 3), up [2, 1] = (4, 5): delta[o][i] = up[o] down[i]."""
    w0 = np.array([[1, 2, 3], [4, 5, 6]], np.float32)
    down, up = np.array([[1, 2]], np.float32), np.array([[3], [4], [5]], np.float32)
    c = L.coef(0.5, 4.0, 1)                                          # 0.5 * 4 / 1 = 2
    assert c == np.float32(2.0)
    got = L.merge_f64(w0, [(down, up, c)])
    assert np.array_equal(got, np.array([[1 + 2 * 3, 2 + 2 * 4, 3 + 2 * 5], [4 + 2 * 6, 5 + 2 * 8, 6 + 2 * 10]], np.float64))
    w0c = w0.reshape(2, 3, 1, 1)
    downc, upc = np.array([1, 2, 3], np.float32).reshape(1, 3, 1, 1), np.array([[4], [5]], np.float32)
    gotc = L.merge_f64(w0c, [(downc, upc, np.float32(-1.0))])
    assert np.array_equal(gotc.reshape(2, 3), np.array([[1 - 4, 2 - 8, 3 - 12], [4 - 5, 5 - 10, 6 - 15]], np.float64))
    # two adapters add; a zero coefficient is skipped; the bound is zero only where nothing is summed
    both = L.merge_f64(w0, [(down, up, c), (down, up, np.float32(-2.0)), (down, up, np.float32(0.0))])
    assert np.array_equal(both, w0.astype(np.float64))
    b = L.merge_bound(w0, [(down, up, c), (down, up, np.float32(0.0))])
    assert np.allclose(b, (1 + 1 + 2) * 2.0 ** -24 * (np.abs(w0) + 2 * np.abs(L.delta_f64(w0.shape, down, up))))


def test_coefficient_is_formed_in_f64_then_rounded():
    assert L.coef(0.7, 8.0, 16) == np.float32(0.7 * 8.0 / 16)
    assert L.coef(-1.3, 2.5, 5) == np.float32(-1.3 * 2.5 / 5)
    assert L.coef(1.0, np.float32(0.1), 3) == np.float32(float(np.float32(0.1)) / 3)    # alpha crosses the C ABI as a float


def test_make_adapter_scale_and_provider():
    d = O.Dims(160, 4, 64, 16, 16, 32)
    base = syn.SyntheticWeights()
    targets = L.arithmetic_targets(d)
    ad = L.make_adapter(targets, 5)
    for name, (shape, rank) in targets.items():
        down, up, alpha = ad[name]
        assert down.shape[0] == rank and up.shape[1] == rank and alpha == rank / 2
        fan = int(np.prod(shape[1:])) if len(shape) == 4 else shape[0]
        w0 = base.get(name, shape, "w", fan)
        dl = float(L.coef(1.0, alpha, rank)) * L.delta_f64(shape, down, up)
        ratio = np.sqrt((dl ** 2).mean()) / np.sqrt((w0.astype(np.float64) ** 2).mean())
        assert 0.03 < ratio < 0.3, (name, ratio)                      # |delta| of the order of 0.1 |W0| (rank-1 factors scatter most)
    prov = L.LoraProvider(base, [(ad, 0.7)])
    name, (shape, rank) = next(iter(targets.items()))
    fan = int(np.prod(shape[1:]))
    merged = prov.get(name, shape, "w", fan)
    assert merged.dtype == np.float32 and not np.array_equal(merged, base.get(name, shape, "w", fan))
    assert np.array_equal(prov.get("unet/lin2_time_embed/weight", (640, 640), "w", 640), base.get("unet/lin2_time_embed/weight", (640, 640), "w", 640))


def test_npz_round_trip(tmp_path):
    from stable_diffusion_burn_amd import load_lora_npz, save_lora_npz
    d = O.Dims(160, 4, 64, 16, 16, 32)
    ad = L.make_adapter(L.repack_targets(d), 9)
    path = tmp_path / "adapter.npz"
    save_lora_npz(path, ad)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(f"{t}::{p}" for t in ad for p in ("down", "up", "alpha"))
    back = load_lora_npz(path)
    assert sorted(back) == sorted(ad)
    for t, (down, up, alpha) in ad.items():
        assert np.array_equal(back[t][0], down) and np.array_equal(back[t][1], up) and back[t][2] == alpha
        assert back[t][0].dtype == np.float32
    np.savez(tmp_path / "bad.npz", **{"a/weight::down": np.zeros((1, 2), np.float32)})
    with pytest.raises(ValueError, match="lacks"):
        load_lora_npz(tmp_path / "bad.npz")
    np.savez(tmp_path / "bad2.npz", **{"a/weight": np.zeros((1, 2), np.float32)})
    with pytest.raises(ValueError, match="unexpected entry"):
        load_lora_npz(tmp_path / "bad2.npz")


class _Recorder:
    """stands where libsdmi would: any call is recorded (and would return success)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


def _fake_sd():
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    sd = StableDiffusion.__new__(StableDiffusion)
    sd._lib, sd.config, sd._ctx, sd._owned = _Recorder(), ModelConfig(64, 1, 32, 8, 8, 32), C.c_void_p(1), False
    specs = [("unet/a/query/weight", (64, 96)), ("unet/a/conv/weight", (32, 64, 3, 3)), ("unet/a/conv/bias", (32,)), ("unet/a/norm/weight", (64,)),
             ("clip/token_embedding/weight", (100, 32)), ("autoencoder/encoder/conv_in/weight", (32, 3, 3, 3)), ("alphas_cumprod", (1000,))]
    sd.weight_specs = lambda: specs
    return sd


def test_python_layer_validates_before_calling_in():
    sd = _fake_sd()
    z = np.zeros
    good_lin = (z((4, 64), np.float32), z((96, 4), np.float32), 4.0)
    good_conv = (z((2, 64, 3, 3), np.float32), z((32, 2), np.float32), 1.0)
    bad = [
        ({}, "non-empty"),
        ({"unet/nope/weight": good_lin}, "not a tensor"),
        ({"unet/a/norm/weight": good_lin}, "not a conv or Linear"),
        ({"unet/a/conv/bias": good_lin}, "not a conv or Linear"),
        ({"clip/token_embedding/weight": good_lin}, "not a conv or Linear"),
        ({"alphas_cumprod": good_lin}, "not a conv or Linear"),
        ({"autoencoder/encoder/conv_in/weight": (z((2, 3, 3, 3), np.float32), z((32, 2), np.float32), 1.0)}, "3-channel"),
        ({"unet/a/query/weight": (z((4, 96), np.float32), z((96, 4), np.float32), 4.0)}, "down must be"),      # down over the OUT features
        ({"unet/a/query/weight": (z((4, 64), np.float32), z((4, 96), np.float32), 4.0)}, "up must be"),        # up transposed
        ({"unet/a/query/weight": (z((4, 64), np.float32), z((96, 3), np.float32), 4.0)}, "up must be"),        # ranks disagree
        ({"unet/a/conv/weight": (z((2, 64 * 9), np.float32), z((32, 2), np.float32), 1.0)}, "down must be"),   # flattened conv factor
        ({"unet/a/query/weight": (z((0, 64), np.float32), z((96, 0), np.float32), 4.0)}, "rank"),
        ({"unet/a/query/weight": (z((257, 64), np.float32), z((96, 257), np.float32), 4.0)}, "rank"),
        ({"unet/a/query/weight": (good_lin[0], good_lin[1], float("nan"))}, "alpha"),
        ({"unet/a/query/weight": (good_lin[0], good_lin[1], float("inf"))}, "alpha"),
        ({"unet/a/query/weight": (good_lin[0], good_lin[1])}, "expected"),
    ]
    for tensors, msg in bad:
        with pytest.raises(ValueError, match=msg):
            sd.lora_attach(tensors)
    for s in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale"):
            sd.lora_attach({"unet/a/query/weight": good_lin}, scale=s)
    with pytest.raises(ValueError, match="not a tensor"):
        sd.effective_weight("unet/nope/weight")
    assert sd._lib.calls == [], sd._lib.calls                   # nothing reached the library
    # ... and a valid adapter goes create -> add per target -> set_scale; a non-finite scale later is caught here too; detach destroys once
    a = sd.lora_attach({"unet/a/query/weight": good_lin, "unet/a/conv/weight": good_conv}, scale=0.5)
    assert sd._lib.calls == ["sdmi_lora_create", "sdmi_lora_add", "sdmi_lora_add", "sdmi_lora_set_scale"]
    with pytest.raises(ValueError, match="scale"):
        a.set_scale(float("nan"))
    a.detach()
    a.detach()
    assert sd._lib.calls[4:] == ["sdmi_lora_destroy"]
    with pytest.raises(ValueError, match="detached"):
        a.set_scale(1.0)


def test_bindings_declare_the_lora_symbols():
    from stable_diffusion_burn_amd import _capi
    header = (ROOT / "include" / "sdmi.h").read_text()
    rust = (ROOT / "ffi" / "sdmi.rs").read_text()
    integ = (ROOT / "INTEGRATION.md").read_text()
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", header), s
        assert s in _capi.SIGNATURES, s
        assert re.search(rf"\bfn {s}\s*\(", rust), s
        assert s in integ, s
    assert re.search(r"pub fn lora_attach\s*\(", rust)
    lib = _capi.load_library()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    design = (ROOT / "DESIGN.md").read_text()
    assert "keep_masters" in design and "9c" in design


def test_merge_kernel_code_object():
    """k_lora.hip as built: no scratch (no spilled register), 16-byte loads and stores of the weight, the factors through LDS"""
    obj = BUILD / "k_lora.hip.o"
    if not obj.exists() or not (LLVM / "llvm-objdump").exists():
        pytest.skip("needs the built object (python -m stable_diffusion_burn_amd.build) and ROCm's llvm tools")
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        fat, dev = Path(td) / "k.fat", Path(td) / "k.co"
        subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(obj), str(Path(td) / "copy.o")], check=True)
        subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={dev}"], check=True)
        text = subprocess.run([str(LLVM / "llvm-objdump"), "-d", str(dev)], check=True, capture_output=True, text=True).stdout
    funcs = {m.group(1): m.group(2) for m in re.finditer(r"^[0-9a-f]+ <(\w+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M)}
    kernels = {k: v for k, v in funcs.items() if "lora_merge_kernel" in k}
    assert len(kernels) == 1, sorted(funcs)
    body = next(iter(kernels.values()))
    assert "scratch_" not in body
    assert "global_load_dwordx4" in body and "global_store_dwordx4" in body and "ds_read_b128" in body
    assert "atomic" not in body


def test_parity_adapter_moves_the_oracle_far_beyond_the_parity_bars():
    """The GPU parity test asserts that its adapter changes the output by more than 100 x its bars (1e-4 on the UNet, 1e-3 on the 3-step latent).  Here the
    reference alone says so: fp32 oracle, adapted (LoraProvider) against un-adapted, the GPU test's inputs."""
    d = O.Dims(160, 4, 64, 16, 16, 32)
    base = syn.SyntheticWeights(cache=True)
    prov = L.LoraProvider(base, [(L.make_adapter(L.parity_targets(d), L.PARITY_SEED), L.PARITY_SCALE)])
    a = syn.alphas_cumprod()
    o0, o1 = O.StableDiffusionOracle(base, a, d, torch.float32), O.StableDiffusionOracle(prov, a, d, torch.float32)
    lat = torch.from_numpy(np.stack([syn.initial_latent(i, 16, 16) for i in range(2)]))
    ctx = torch.from_numpy(np.stack([syn.cond_context(i, 7, 64) for i in range(2)]))
    unc = torch.from_numpy(syn.uncond_context(2, 64))
    for t in (999, 49):
        diff = float((o0.unet.forward(lat, t, ctx) - o1.unet.forward(lat, t, ctx)).abs().max())
        print(f"t = {t}: max |adapted - base| = {diff:.3e}")
        assert diff > 100 * 1e-4
    diff = float((o0.sample_latent(ctx[:1], unc, 7.5, 3, lat[:1]) - o1.sample_latent(ctx[:1], unc, 7.5, 3, lat[:1])).abs().max())
    print(f"3-step latent: max |adapted - base| = {diff:.3e}")
    assert diff > 100 * 1e-3
