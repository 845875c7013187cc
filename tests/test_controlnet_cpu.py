"""ControlNet for SD v1 (include/sdmi.h "ControlNet"), the parts that need no GPU: the reference in tests/controlnet_ref.py against
the plain oracle, the checkpoint key rules against tests/golden/controlnet_ckpt_keys.txt, the step-window rule, the cldm-layout writer, the bindings."""
import ctypes as C
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import controlnet_ref as CR
from oracle import sd_oracle as O

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "controlnet_ckpt_keys.txt"
SMALL = O.Dims(model_channels=32, n_head=1, ctx_dim=32, latent_h=8, latent_w=8, vae_ch=32)
NEW_SYMBOLS = ("sdmi_load_control_safetensors", "sdmi_control_ready", "sdmi_set_control", "sdmi_control_step_on", "sdmi_control_hint_embed",
               "sdmi_control_residuals_size", "sdmi_control_residuals")


@pytest.fixture(scope="module")
def sdmi():
    from stable_diffusion_burn_amd import build
    build.build(force=False, verbose=False)
    import stable_diffusion_burn_amd as pkg
    return pkg


class ZeroedZeroConvs:
    """a provider whose zero convolutions and middle_block_out are all zeros: what a freshly initialised ControlNet holds"""

    def __init__(self, base):
        self.base = base

    def get(self, name, shape, kind, fan_in=0):
        if name.startswith("controlnet/zero_convs/") or name.startswith("controlnet/middle_block_out/"):
            return np.zeros(tuple(shape), np.float32)
        return self.base.get(name, shape, kind, fan_in)


def _inputs(d, n=2, T=5):
    g = np.random.default_rng(5)
    x = torch.from_numpy(g.standard_normal((n, 4, d.latent_h, d.latent_w)).astype(np.float32))
    ctx = torch.from_numpy(g.standard_normal((n, T, d.ctx_dim)).astype(np.float32))
    hint = g.integers(0, 256, (n, 8 * d.latent_h, 8 * d.latent_w, 3), dtype=np.uint8)
    return x, ctx, hint


def test_zero_convolutions_make_the_control_an_identity(synth):
    x, ctx, hint = _inputs(SMALL)
    unet = O.UNetOracle(synth, SMALL, torch.float64)
    r = CR.ControlNetOracle(ZeroedZeroConvs(synth), SMALL, torch.float64).forward(x, 500, ctx, CR.hint01(hint))
    assert len(r) == 13 and all(float(v.abs().max()) == 0.0 for v in r)
    assert torch.equal(CR.controlled_forward(unet, x, 500, ctx, r, 1.0), unet.forward(x, 500, ctx))
    assert torch.equal(CR.controlled_forward(unet, x, 500, ctx, None, 1.0), unet.forward(x, 500, ctx))


def test_residual_shapes_and_the_hint_reach_the_output(synth, sdmi):
    from stable_diffusion_burn_amd.pipeline import control_residual_shapes
    d = SMALL
    x, ctx, hint = _inputs(d)
    unet, ctl = O.UNetOracle(synth, d, torch.float64), CR.ControlNetOracle(synth, d, torch.float64)
    r = ctl.forward(x, 500, ctx, CR.hint01(hint))
    want = [(2, c, d.latent_h >> s, d.latent_w >> s) for c, s in control_residual_shapes(d.model_channels)]
    assert [tuple(v.shape) for v in r] == want
    emb = ctl.hint_embed(CR.hint01(hint))
    assert tuple(emb.shape) == (2, d.model_channels, d.latent_h, d.latent_w)
    plain = unet.forward(x, 500, ctx)
    steered = CR.controlled_forward(unet, x, 500, ctx, r, 0.6)
    assert float((steered - plain).abs().max()) > 1e-3
    # one hint for the batch == that hint given once per image
    one = ctl.forward(x, 500, ctx, CR.hint01(hint[:1]))
    two = ctl.forward(x, 500, ctx, CR.hint01(np.repeat(hint[:1], 2, 0)))
    assert all(float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())) for a, b in zip(one, two))   # (fp64; a batch-1 convolution may sum in another order)


def fixture_rows():
    rows = [ln.split("\t") for ln in FIXTURE.read_text().splitlines()]
    assert all(len(r) == 4 for r in rows)
    return [(d, k, tuple(int(v) for v in s.split(",")), t == "T") for d, k, s, t in rows]


def test_key_map_reproduces_the_fixture(sdmi, tmp_path):
    """tests/golden/controlnet_ckpt_keys.txt holds names only, WRITTEN BY THE RULE (no ControlNet file exists offline): this guards against drift, it is no proof.
    The encoder part shares its rules with the pinned UNet map: every such key is the UNet's with another root."""
    from stable_diffusion_burn_amd import weights as W
    rows = fixture_rows()
    specs = W.control_specs(O.Dims())
    assert len(rows) == len(specs) == 340
    for (name, shape), (dump, key, kshape, tr) in zip(specs, rows):
        assert name == dump
        got_key, got_tr = sdmi.checkpoint_key(name)
        assert (got_key, got_tr) == (key, tr), name
        assert (tuple(reversed(shape)) if tr else tuple(shape)) == kshape, name
        if not re.match(r"controlnet/(hint|zero_convs|middle_block_out)", name):
            ukey, utr = sdmi.checkpoint_key("unet/" + name[len("controlnet/"):])
            assert ukey == "model.diffusion_model." + key[len("control_model."):] and utr == tr, name
    assert len({k for _, k, _, _ in rows}) == len(rows)
    # the inverse, through the listing of a file that holds every key (one float each: the listing does not look at shapes)
    path = tmp_path / "keys.safetensors"
    W.write_safetensors(path, {k: np.zeros(1, np.float32) for _, k, _, _ in rows} | {"control_model.input_hint_block.1.weight": np.zeros(1, np.float32)})
    listed = {key: name for key, _, _, _, name in sdmi.safetensors_list(path)}
    for dump, key, _, _ in rows:
        assert listed[key] == dump
    assert listed["control_model.input_hint_block.1.weight"] is None
    # what a ControlNet does not have has no key
    for bad in ("controlnet/output_blocks/r1/conv_in/weight", "controlnet/norm_out/weight", "controlnet/conv_out/bias", "controlnet/hint/c8/weight",
                "controlnet/zero_convs/12/weight", "controlnet/zero_convs/01/weight", "controlnet/middle_block_out/0/weight", "controlnet/hint/c0/stride"):
        with pytest.raises(sdmi.SdmiError):
            sdmi.checkpoint_key(bad)


WINDOW_TABLE = [
    # S, start, end -> controlled step indices
    (4, 0.25, 0.75, [1, 2]),
    (4, 0.0, 1.0, [0, 1, 2, 3]),
    (4, 0.0, 0.0, []),
    (4, 1.0, 1.0, []),
    (4, 0.5, 0.5, []),
    (2, 0.0, 0.5, [0]),                 # an img2img tail of 2 steps: the window counts the tail's own steps
    (5, 0.3, 0.7, [2, 3]),              # 1.5 <= i < 3.5
    (10, 0.1, 0.3, [1, 2]),             # 0.1 * 10 == 1.0 and 0.3 * 10 == 3.0 in f64: step 1 is in, step 3 is out
    (3, 1 / 3, 1.0, [1, 2]),            # (1/3) * 3 == 1.0 exactly in f64: step 1 is controlled
    (3, 0.0, 1 / 3, [0]),               # and step 1 is not below 1.0
    (3, 0.33, 0.67, [1, 2]),            # 0.99 <= i < 2.01
    (1, 0.0, 1.0, [0]),
    (1, 0.5, 1.0, []),                  # 0.5 <= 0 is false
]


def test_step_window_rule(sdmi):
    # the f64 products the table leans on, spelled out
    assert (1 / 3) * 3 == 1.0 and 0.1 * 10 == 1.0 and 0.3 * 10 == 3.0
    for S, start, end, want in WINDOW_TABLE:
        got = [i for i in range(S) if sdmi.control_step_on(start, end, i, S)]
        assert got == want == CR.window(start, end, S), (S, start, end, got)
    lib = sdmi._capi.load_library()
    for bad in ((0.5, 0.25, 0, 4), (-0.1, 1.0, 0, 4), (0.0, 1.5, 0, 4), (float("nan"), 1.0, 0, 4), (0.0, 1.0, 4, 4), (0.0, 1.0, 0, 0)):
        assert lib.sdmi_control_step_on(*bad) == -1


def _read_safetensors(path):
    raw = Path(path).read_bytes()
    n = int.from_bytes(raw[:8], "little")
    header = json.loads(raw[8:8 + n])
    out = {}
    for key, info in header.items():
        b, e = info["data_offsets"]
        dt = {"F32": np.float32, "F16": np.float16}[info["dtype"]]
        out[key] = np.frombuffer(raw[8 + n + b:8 + n + e], dt).reshape(info["shape"])
    return out


@pytest.mark.parametrize("dtype", ["F32", "F16"])
def test_writer_round_trip(sdmi, synth, tmp_path, dtype):
    """write_control_safetensors is the inverse of the loader's map: numpy alone reads back every tensor, Linear weights as torch's [out, in]"""
    from stable_diffusion_burn_amd import synthetic as syn
    from stable_diffusion_burn_amd import weights as W
    specs = W.control_specs(SMALL)
    shapes = dict(specs)
    path = tmp_path / f"control_{dtype}.safetensors"
    W.write_control_safetensors(path, synth, SMALL, dtype)
    back = _read_safetensors(path)
    assert len(back) == len(specs) == 340 and all(k.startswith("control_model.") for k in back)
    for name, shape in specs:
        key, tr = sdmi.checkpoint_key(name)
        want = syn.named_tensor(synth, name, shape, shapes)
        want = want.T if tr else want
        if dtype == "F16":
            want = want.astype(np.float16)
        assert back[key].dtype == want.dtype and np.array_equal(back[key], want), name
    # a dict of tensors in the dump's layout is taken the same way; a wrong shape is refused
    tensors = {name: syn.named_tensor(synth, name, shape, shapes) for name, shape in specs}
    W.write_control_safetensors(tmp_path / "again.safetensors", tensors, SMALL, dtype)
    assert (tmp_path / "again.safetensors").read_bytes() == path.read_bytes()
    tensors["controlnet/zero_convs/3/weight"] = np.zeros((1, 1, 1, 1), np.float32)
    with pytest.raises(ValueError):
        W.write_control_safetensors(tmp_path / "bad.safetensors", tensors, SMALL, dtype)


def test_symbols_and_bindings(sdmi):
    from stable_diffusion_burn_amd import ModelConfig, StableDiffusion
    from stable_diffusion_burn_amd._capi import SIGNATURES, SdmiConfig, SdmiControl
    lib = sdmi._capi.load_library()
    header = (ROOT / "include" / "sdmi.h").read_text()
    rs = (ROOT / "ffi" / "sdmi.rs").read_text()
    for s in NEW_SYMBOLS:
        assert s in SIGNATURES and getattr(lib, s).argtypes == SIGNATURES[s][1], s
        assert re.search(rf"\b(int|int64_t) {s}\s*\(", header), s
        assert re.search(rf"\bfn {s}\s*\(", rs), s
    assert C.sizeof(SdmiControl) == 8 + 3 * 4 + 4 + 3 * 8 + 4 * 8 and SdmiControl.strength.offset == 24
    assert re.search(r"pub struct SdmiControl", rs) and re.search(r"int32_t control_hint_ch;", header)
    # the field is the first reserved word: the struct's size and every earlier offset stay
    cfg = SdmiConfig()
    assert lib.sdmi_default_config(C.byref(cfg)) == 0 and cfg.control_hint_ch == 0 and C.sizeof(SdmiConfig) == 64
    cfg.control_hint_ch = 3
    assert cfg.reserved[0] == 3 and SdmiConfig.reserved.offset == 56
    assert ModelConfig().control_hint_ch == 0 and ModelConfig(control_hint_ch=3).control_hint_ch == 3
    for name in ("set_control", "control_hint_embed", "control_residuals", "load_control_safetensors"):
        assert callable(getattr(StableDiffusion, name))
