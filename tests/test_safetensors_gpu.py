"""SD v1.x .safetensors checkpoints loaded natively and converted on the device (include/sdmi.h: sdmi_load_weights_safetensors).

What is pinned here, everything bit for bit: the conversion kernel alone (csrc/k_unpack.hip through sdmi_op_unpack_tensor) against numpy on every dtype,
transform and code path; a whole model written in the CHECKPOINT's naming by weights.write_checkpoint_safetensors -- the key names taken from the fixture the
reference's Python side wrote (tests/golden/sd14_ckpt_keys.txt), not from the library -- against a second context that received the same values through
set_weight; every status of the header; the computed schedule; the multi-device surface.

Configurations: precision 0 runs the half-width model of tests/test_lora_gpu.py with its CLIP group (1 layer, 1 head, 48 tokens, 8 positions) and the VAE
encoder.  The bf16 / MXFP8 kernels need channel counts that are multiples of 64 (tests/test_bf16_gpu.py), so precision 1 and 2 run the full-width model at
an 8 x 8 latent as every other module does; its text width is 768, which one head cannot serve (the fused attention's head dims are 40 / 64 / 80 / 160), so
there the CLIP group has 12 heads -- the same head dim, 64, as the half-width model's one.  Files and contexts are made once per module and shared.
"""
import json
import shutil
from pathlib import Path

import numpy as np
import pytest

import lora_ref as L
from oracle import sd_oracle as O
from stable_diffusion_burn_amd import ModelConfig, MultiStableDiffusion, SdmiError, StableDiffusion
from stable_diffusion_burn_amd import synthetic as syn
from stable_diffusion_burn_amd import weights as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
WIDE = O.Dims(320, 8, 768, 8, 8, 64)
ERR_WEIGHTS, ERR_IO, ERR_UNSUPPORTED, ERR_STATE = -3, -4, -5, -6
FIXTURE = {d: (k, t == "T") for d, k, _, t in (ln.split("\t") for ln in (ROOT / "tests" / "golden" / "sd14_ckpt_keys.txt").read_text().splitlines())}
EXTRA = {"model_ema.decay": np.array(0.9999, np.float32), "model_ema.diffusion_modelout2weight": np.ones((4, 5), np.float32),
         "cond_stage_model.transformer.text_model.embeddings.position_ids": np.arange(8, dtype=np.int64)[None]}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the kernel alone --------------------------------------------------------------------------------------------------------------------------
# +-0, the smallest and the largest subnormal, the smallest normal, the maximum, +-inf, a quiet and a signalling NaN
SPECIAL = {"F16": [0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0x0200, 0x02AB],
           "BF16": [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x7F80, 0xFF80, 0x7FC0, 0x7F81, 0x0040, 0x0055],
           "F32": [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                   0x7FC00000, 0x7F800001, 0x00400000, 0x00555555]}


def _raw(dtype, shape, seed):
    """random BIT PATTERNS of the dtype (every exponent, subnormals and NaNs included) with the special values spread over the tensor"""
    g = np.random.default_rng(seed)
    n = int(np.prod(shape))
    a = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) if dtype == "F32" else g.integers(0, 1 << 16, n, dtype=np.uint32).astype(np.uint16)
    k = min(n, len(SPECIAL[dtype]))
    a[np.arange(k) * (n // k)] = np.array(SPECIAL[dtype][:k], a.dtype)
    a = a.reshape(shape)
    if dtype == "F32":
        return a.view(np.float32), a.view(np.float32)
    if dtype == "F16":
        return a.view(np.float16), a.view(np.float16).astype(np.float32)
    return a, W.bf16_to_f32(a)


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# the issue's shapes + (72, 136) / (128, 192): 16-byte pieces on both sides with partial and with several whole tiles; (4, 2056): vector rows longer than one tile
SHAPES_2D = [(1, 1), (1, 77), (77, 1), (33, 70), (64, 64), (65, 129), (7, 2049), (72, 136), (128, 192), (4, 2056), (68, 60)]


@pytest.mark.parametrize("dtype", ["F32", "F16", "BF16"])
@pytest.mark.parametrize("shape", SHAPES_2D)
def test_kernel_2d_copy_and_transpose(sd_ops, dtype, shape):
    raw, want = _raw(dtype, shape, 11)
    _same(sd_ops.op_unpack_tensor(raw, dtype, 0), want)
    _same(sd_ops.op_unpack_tensor(raw, dtype, 1), np.ascontiguousarray(want.T))


@pytest.mark.parametrize("dtype", ["F32", "F16", "BF16"])
def test_kernel_other_ranks_and_the_channel_pad(sd_ops, dtype):
    raw, want = _raw(dtype, (5, 4, 3, 3), 12)
    _same(sd_ops.op_unpack_tensor(raw, dtype, 0), want)
    raw, want = _raw(dtype, (5, 3, 3, 3), 13)
    _same(sd_ops.op_unpack_tensor(raw, dtype, 0), want)
    padded = np.zeros((5, 4, 3, 3), np.float32)
    padded[:, :3] = want
    got = sd_ops.op_unpack_tensor(raw, dtype, 2)
    _same(got, padded)
    assert not np.signbit(got[:, 3]).any()                    # the 4th channel is +0
    raw, want = _raw(dtype, (3,), 14)
    _same(sd_ops.op_unpack_tensor(raw, dtype, 0), want)
    raw, want = _raw(dtype, (len(SPECIAL[dtype]),), 15)          # every special value, in order
    got = sd_ops.op_unpack_tensor(raw, dtype, 0)
    _same(got, want)
    assert np.isnan(got[11]) and np.isnan(got[12]) and np.isinf(got[9]) and got[9] > 0 and np.isinf(got[10]) and got[10] < 0
    assert np.signbit(got[1]) and got[1] == 0 and not np.signbit(got[0])
    if dtype == "F16":
        assert got[2] == 2.0 ** -24 and got[3] == -(2.0 ** -24) and got[4] == 1023 * 2.0 ** -24 and got[6] == 2.0 ** -14 and got[7] == 65504.0
    raw, want = _raw(dtype, (4099,), 16)                         # a vector body and a scalar tail
    _same(sd_ops.op_unpack_tensor(raw, dtype, 0), want)


@pytest.mark.parametrize("dtype", ["F16", "BF16"])
def test_kernel_every_16_bit_pattern(sd_ops, dtype):
    """all 65 536 bit patterns as one [256, 256] tensor, copied and transposed: numpy's values for everything but NaN, and for NaN the payload kept as it is
    (sign, the mantissa bits moved up, nothing quieted) -- the integer form of both conversions"""
    bits = np.arange(65536, dtype=np.uint32)
    raw = bits.astype(np.uint16).reshape(256, 256)
    if dtype == "F16":
        want = raw.view(np.float16).astype(np.float32)
        nan_bits = ((bits & 0x8000) << 16) | 0x7F800000 | ((bits & 0x3FF) << 13)
        raw = raw.view(np.float16)
    else:
        want = W.bf16_to_f32(raw)
        nan_bits = bits << 16
    nan = np.isnan(want)
    assert nan.sum() == (2046 if dtype == "F16" else 254)
    want_bits = np.where(nan, nan_bits.reshape(256, 256), _bits(want)).astype(np.uint32)
    assert np.array_equal(_bits(sd_ops.op_unpack_tensor(raw, dtype, 0)), want_bits)
    assert np.array_equal(_bits(sd_ops.op_unpack_tensor(raw, dtype, 1)), np.ascontiguousarray(want_bits.T))


def test_kernel_argument_errors(sd_ops):
    x = np.zeros((2, 3), np.float32)
    for bad in (lambda: sd_ops.op_unpack_tensor(np.zeros((2, 3, 4), np.float32), "F32", 1), lambda: sd_ops.op_unpack_tensor(np.zeros((2, 4, 3, 3), np.float32), "F32", 2),
                lambda: sd_ops.op_unpack_tensor(x, "F32", 3)):
        with pytest.raises(SdmiError) as ei:
            bad()
        assert ei.value.status == -1
    _same(sd_ops.op_unpack_tensor(x + 1, "F32", 1), np.ones((3, 2), np.float32))


# ---- whole model ---------------------------------------------------------------------------------------------------------------------------------
def _dims(precision, tiny_dims):
    return tiny_dims if precision == 0 else WIDE


def _config(d, precision):
    return ModelConfig(d.model_channels, d.n_head, d.ctx_dim, d.latent_h, d.latent_w, d.vae_ch, precision=precision,
                       clip_layers=1, clip_heads=d.ctx_dim // 64, clip_vocab=48, clip_ctx=8)


def _new(d, precision):
    sd = StableDiffusion(_config(d, precision))
    sd.set_option("keep_masters", 1)
    return sd


def _round(a, dtype):
    """what the checkpoint holds, as float32"""
    a = np.asarray(a, np.float32)
    return a if dtype == "F32" else a.astype(np.float16).astype(np.float32) if dtype == "F16" else W.bf16_to_f32(W.bf16_bits(a))


@pytest.fixture(scope="module")
def model(synth, tiny_dims, tmp_path_factory):
    """files(wide, dtype) -> a checkpoint written once; pair(precision) -> (context for the file loader, context for set_weight), made once"""
    root = tmp_path_factory.mktemp("ckpt")
    files, pairs, specs = {}, {}, {}

    def spec_of(wide):
        if wide not in specs:
            sd = StableDiffusion(_config(WIDE if wide else tiny_dims, 0))
            specs[wide] = sd.weight_specs()
            sd.close()
        return specs[wide]

    def file(wide, dtype):
        if (wide, dtype) not in files:
            sp = spec_of(wide)
            shapes = dict(sp)
            path = root / f"{'wide' if wide else 'tiny'}_{dtype}.safetensors"
            W.write_checkpoint_safetensors(path, sp, lambda n, s: syn.named_tensor(synth, n, s, shapes), syn.alphas_cumprod(1000), dtype=dtype,
                                           key_of=lambda n: FIXTURE[n], extra=EXTRA)
            files[(wide, dtype)] = path
        return files[(wide, dtype)]

    def pair(precision):
        if precision not in pairs:
            d = _dims(precision, tiny_dims)
            pairs[precision] = (_new(d, precision), _new(d, precision))
        return pairs[precision]

    class M:
        pass
    M.file, M.pair, M.specs = staticmethod(file), staticmethod(pair), staticmethod(spec_of)
    yield M
    for a, b in pairs.values():
        a.close()
        b.close()
    shutil.rmtree(root, ignore_errors=True)


def _inputs(d):
    g = np.random.default_rng(9)
    return {"lat": np.stack([syn.initial_latent(i, d.latent_h, d.latent_w) for i in range(2)]),
            "ctx": np.stack([syn.cond_context(i, 7, d.ctx_dim) for i in range(2)]),
            "img": g.uniform(-1, 1, (1, 3, 8 * d.latent_h, 8 * d.latent_w)).astype(np.float32),
            "tok": g.integers(0, 48, (2, 8)).astype(np.int32)}


def _outputs(sd, d):
    x = _inputs(d)
    return {"unet_forward": sd.unet.forward(x["lat"], [500], x["ctx"]), "decode_latent": sd.autoencoder.decode_latent(x["lat"][:1]),
            "encode_image": sd.autoencoder.encode_image(x["img"]), "clip_forward": sd.clip.forward(x["tok"])}


def _is_matrix_weight(name, shape):
    return len(shape) == 4 or (len(shape) == 2 and "embedding" not in name)


@pytest.mark.parametrize("precision,dtype", [(0, "F32"), (0, "F16"), (0, "BF16"), (1, "F32"), (1, "F16"), (1, "BF16"), (2, "F16")])
def test_checkpoint_equals_set_weight(model, synth, tiny_dims, precision, dtype):
    d = _dims(precision, tiny_dims)
    specs = model.specs(precision != 0)
    shapes = dict(specs)
    A, B = model.pair(precision)
    A.load_weights_safetensors(model.file(precision != 0, dtype))
    for name, shape in specs:
        B.set_weight(name, syn.alphas_cumprod(1000) if name == "alphas_cumprod" else _round(syn.named_tensor(synth, name, shape, shapes), dtype))
    assert B._lib.sdmi_finalize_weights(B._ctx) == 0
    checked = 0
    for name, shape in specs:
        if not _is_matrix_weight(name, shape):
            continue
        a, b = A.effective_weight(name), B.effective_weight(name)
        assert np.array_equal(_bits(a), _bits(b)), f"{name} ({FIXTURE[name][0]}) differs: a wrong key or a wrong transpose"
        checked += 1
    assert checked > 300 and np.isfinite(A.effective_weight("unet/conv_out/weight")).all()
    oa, ob = _outputs(A, d), _outputs(B, d)
    for k in oa:
        assert np.isfinite(oa[k]).all() and np.abs(oa[k]).max() > 0, k
        assert np.array_equal(_bits(oa[k]), _bits(ob[k])), k


def test_every_weight_name_is_in_the_fixture(model):
    names = [n for n, _ in model.specs(False)]
    assert len(names) > 900
    missing = [n for n in names if n not in FIXTURE and n != "alphas_cumprod"]
    assert not missing, missing[:5]
    assert [n for n, _ in model.specs(True)] == names          # the names do not depend on the widths


# ---- errors: variants of the half-width F16 file with an edited header (the data section is reused as it is) ----------------------------------------
def _variant(src, dst, edit, keep=None):
    """dst = src with edit(header) applied; edit returns bytes appended to the data section (or None); keep: truncate the DATA SECTION to that many bytes"""
    with open(src, "rb") as f:
        hlen = int.from_bytes(f.read(8), "little")
        header = json.loads(f.read(hlen))
        end = max(v["data_offsets"][1] for k, v in header.items() if k != "__metadata__")
        tail = edit(header, end) if edit else None
        text = json.dumps(header, separators=(",", ":")).encode()
        with open(dst, "wb") as o:
            o.write(len(text).to_bytes(8, "little") + text)
            if keep is None:
                shutil.copyfileobj(f, o, 16 << 20)
            else:
                o.write(f.read(keep))
            if tail:
                o.write(tail)
    return dst


@pytest.fixture(scope="module")
def loaded(model, tiny_dims):
    """a half-width context loaded from the F16 file, with the outputs the error tests compare against"""
    sd = _new(tiny_dims, 0)
    sd.load_weights_safetensors(model.file(False, "F16"))
    x = _inputs(tiny_dims)
    ref = {"forward": sd.unet.forward(x["lat"], [500], x["ctx"]), "clip": sd.clip.forward(x["tok"])}
    yield sd, ref
    sd.close()


def _still_the_loaded_model(sd, ref, d):
    x = _inputs(d)
    assert np.array_equal(_bits(sd.unet.forward(x["lat"], [500], x["ctx"])), _bits(ref["forward"]))
    assert np.array_equal(_bits(sd.clip.forward(x["tok"])), _bits(ref["clip"]))


def test_missing_hot_path_key(model, loaded, tiny_dims, tmp_path):
    sd, ref = loaded
    dump = "unet/middle_block/res1/conv_in/weight"
    key = FIXTURE[dump][0]
    path = _variant(model.file(False, "F16"), tmp_path / "v.safetensors", lambda h, end: h.__setitem__("unused.tensor", h.pop(key)))
    with pytest.raises(SdmiError) as ei:
        sd.load_weights_safetensors(path)
    print(ei.value)
    assert ei.value.status == ERR_WEIGHTS and dump in str(ei.value) and key in str(ei.value)
    _still_the_loaded_model(sd, ref, tiny_dims)


def test_partial_clip_group_is_refused_at_finalize(model, loaded, tiny_dims, tmp_path):
    ref = loaded[1]
    key = FIXTURE["clip/blocks/0/mlp/fc2/bias"][0]
    path = _variant(model.file(False, "F16"), tmp_path / "v.safetensors", lambda h, end: h.__setitem__("unused.tensor", h.pop(key)))
    sd = _new(tiny_dims, 0)
    try:
        with pytest.raises(SdmiError) as ei:
            sd.load_weights_safetensors(path)
        print(ei.value)
        assert ei.value.status == ERR_WEIGHTS and "CLIP weights are partially set" in str(ei.value) and "clip/blocks/0/mlp/fc2/bias" in str(ei.value)
        sd.load_weights_safetensors(model.file(False, "F16"))
        _still_the_loaded_model(sd, ref, tiny_dims)
    finally:
        sd.close()


def test_wrong_shape(model, loaded, tiny_dims, tmp_path):
    sd, ref = loaded
    key = FIXTURE["unet/lin1_time_embed/weight"][0]
    c = tiny_dims.model_channels

    def edit(h, end):
        assert h[key]["shape"] == [4 * c, c]
        h[key]["shape"] = [c, 4 * c]           # the dump's [in, out] where the checkpoint holds [out, in]: same byte length
    path = _variant(model.file(False, "F16"), tmp_path / "v.safetensors", edit)
    with pytest.raises(SdmiError) as ei:
        sd.load_weights_safetensors(path)
    print(ei.value)
    assert ei.value.status == ERR_WEIGHTS and key in str(ei.value) and f"[{c},{4 * c}]" in str(ei.value) and f"[{4 * c},{c}]" in str(ei.value)
    _still_the_loaded_model(sd, ref, tiny_dims)


def test_f64_on_a_mapped_tensor(model, loaded, tiny_dims, tmp_path):
    sd, ref = loaded
    key = FIXTURE["unet/conv_out/bias"][0]

    def edit(h, end):
        h["unused.tensor"] = h.pop(key)
        h[key] = {"dtype": "F64", "shape": [4], "data_offsets": [end, end + 32]}
        return np.zeros(4, np.float64).tobytes()
    path = _variant(model.file(False, "F16"), tmp_path / "v.safetensors", edit)
    with pytest.raises(SdmiError) as ei:
        sd.load_weights_safetensors(path)
    print(ei.value)
    assert ei.value.status == ERR_UNSUPPORTED and key in str(ei.value) and "F64" in str(ei.value)
    _still_the_loaded_model(sd, ref, tiny_dims)


def test_file_truncated_inside_the_data_section(model, loaded, tiny_dims, tmp_path):
    sd, ref = loaded
    src = model.file(False, "F16")
    hlen = int.from_bytes(open(src, "rb").read(8), "little")
    data = src.stat().st_size - 8 - hlen
    path = _variant(src, tmp_path / "v.safetensors", None, keep=data // 2)
    with pytest.raises(SdmiError) as ei:
        sd.load_weights_safetensors(path)
    print(ei.value)
    assert ei.value.status in (ERR_IO, ERR_WEIGHTS) and "outside the data section" in str(ei.value)
    _still_the_loaded_model(sd, ref, tiny_dims)


def test_bulk_load_under_an_active_adapter(model, loaded, tiny_dims):
    sd, ref = loaded
    a = sd.lora_attach(L.make_adapter(L.repack_targets(tiny_dims), 41), scale=0.5)
    try:
        with pytest.raises(SdmiError) as ei:
            sd.load_weights_safetensors(model.file(False, "F16"))
        assert ei.value.status == ERR_STATE and "LoRA" in str(ei.value)
    finally:
        a.detach()
    _still_the_loaded_model(sd, ref, tiny_dims)


def test_no_matching_key(loaded, tiny_dims, tmp_path):
    sd, ref = loaded
    W.write_safetensors(tmp_path / "other.safetensors", EXTRA)
    with pytest.raises(SdmiError) as ei:
        sd.load_weights_safetensors(tmp_path / "other.safetensors")
    assert ei.value.status == ERR_WEIGHTS
    _still_the_loaded_model(sd, ref, tiny_dims)


def _sample_args(d):
    return syn.cond_context(0, 7, d.ctx_dim)[None], syn.uncond_context(2, d.ctx_dim), syn.initial_latent(0, d.latent_h, d.latent_w)[None]


def test_schedule_is_computed_when_the_file_has_none(model, loaded, tiny_dims, tmp_path):
    sd, _ = loaded
    ctx, unc, lat = _sample_args(tiny_dims)
    want = sd.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    path = _variant(model.file(False, "F16"), tmp_path / "v.safetensors", lambda h, end: h.__setitem__("unused.alphas", h.pop("alphas_cumprod")))
    other = _new(tiny_dims, 0)
    try:
        other.load_weights_safetensors(path)
        got = other.sample_latent(ctx, unc, 7.5, 3, init_latent=lat)
    finally:
        other.close()
    assert np.isfinite(want).all() and np.array_equal(_bits(got), _bits(want))


def test_multi_device_loads_the_same_model(model, loaded, tiny_dims):
    sd, _ = loaded
    ctx, unc, lat = _sample_args(tiny_dims)
    want = sd.sample_image(ctx, unc, 7.5, 2, init_latent=lat)
    m = MultiStableDiffusion(_config(tiny_dims, 0), devices=(0,))
    try:
        m.load_weights_path("safetensors", model.file(False, "F16"))
        got = m.sample_image(ctx, unc, 7.5, 2, 1, init_latents=lat)
        with pytest.raises(SdmiError):
            m.load_weights_path("ckpt", model.file(False, "F16"))
    finally:
        m.close()
    assert got.shape == want.shape and np.array_equal(got, want)
